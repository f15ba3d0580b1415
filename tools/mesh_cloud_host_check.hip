// Host rehearsal of csrc/mesh_cloud.hip: the statements the kernels share with the host (csrc/mesh_cloud_shared.h: tri_setup, rows_of,
// row_candidates, row_point, cell_key, cells_along) run serially on the CPU, triangle by triangle, row by row, candidate by candidate, and the
// winner of every cell is taken as mcloud_winners_kernel takes it (smallest distance bits, then smallest candidate number).  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/mesh_cloud_host_check.hip -o mesh_cloud_host_check
//   mesh_cloud_host_check MESH.bin SPACING OUT.bin       (add -Xarch_host -fsanitize=address,undefined for a checked run)
//
// MESH.bin: int32 nv, int32 nf, nv*3 float32, nf*3 int32.  OUT.bin: int64 candidates, int64 m, m*3 float32 points, m int32 triangles.
// Exit status 3 with a message for what psi_mesh_cloud_count refuses.  It does not cover the kernels' searches in the scans, their atomics
// or the device's division, square root and rounding to integers: those need the GPU tests.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "../psi-release_amd/csrc/mesh_cloud_shared.h"

namespace C = psi_mcloud;

struct Cand {
    int64_t cell;
    uint32_t key;
    int64_t q;
};

static int refuse(const char *why)
{
    fprintf(stderr, "refused: %s\n", why);
    return 3;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s MESH.bin SPACING OUT.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int nv = 0, nf = 0;
    if (fread(&nv, 4, 1, f) != 1 || fread(&nf, 4, 1, f) != 1 || nv < 0 || nf < 0) return 2;
    std::vector<float> hv((size_t)nv * 3);
    std::vector<int32_t> hf((size_t)nf * 3);
    if (fread(hv.data(), 4, hv.size(), f) != hv.size() || fread(hf.data(), 4, hf.size(), f) != hf.size()) return 2;
    fclose(f);
    const float v = (float)atof(argv[2]);
    if (!(std::isfinite(v) && v > 0.0f && C::half_spacing(v) > 0.0f)) return refuse("spacing must be a positive finite fp32 number");
    if (nf < 1 || nv < 1) return refuse("nf >= 1 and nv >= 1");
    const float h = C::half_spacing(v);

    // the count pass: validation, the box of the referenced vertices, rows and candidates
    float lo[3], hi[3];
    bool first = true;
    long long n_rows = 0, n_cands = 0;
    for (int t = 0; t < nf; t++) {
        const float *p[3];
        for (int c = 0; c < 3; c++) {
            const int i = hf[(size_t)t * 3 + c];
            if (i < 0 || i >= nv) return refuse("a face index lies outside [0, nv)");
            p[c] = &hv[(size_t)i * 3];
            for (int k = 0; k < 3; k++) {
                if (!std::isfinite(p[c][k])) return refuse("a vertex coordinate of a triangle is not finite");
                lo[k] = first || p[c][k] < lo[k] ? p[c][k] : lo[k];
                hi[k] = first || p[c][k] > hi[k] ? p[c][k] : hi[k];
            }
            first = false;
        }
        bool too_long;
        const C::Tri tr = C::tri_setup(p[0], p[1], p[2], h, &too_long);
        if (too_long) return refuse("an edge spans more than 2^21 cells");
        const int nr = C::rows_of(tr);
        n_rows += nr;
        for (int r = 0; r < nr; r++) n_cands += C::row_candidates(tr, r, h);
    }
    float o[3];
    for (int k = 0; k < 3; k++) {
        if (!(C::cells_along(lo[k], hi[k], h, v) <= (float)C::MAX_CELLS)) return refuse("more than 2^21 cells along an axis");
        o[k] = C::cell_origin(lo[k], h);
    }
    if (n_cands < 1) return refuse("no triangle with area");
    if (n_cands > C::MAX_CANDIDATES) return refuse("more than 2^31 - 1 candidates");

    // the emit pass, in candidate order
    std::vector<float> pos((size_t)n_cands * 3);
    std::vector<int32_t> tri((size_t)n_cands);
    std::vector<Cand> cand((size_t)n_cands);
    int64_t q = 0;
    for (int t = 0; t < nf; t++) {
        bool too_long;
        const C::Tri tr = C::tri_setup(&hv[(size_t)hf[(size_t)t * 3] * 3], &hv[(size_t)hf[(size_t)t * 3 + 1] * 3], &hv[(size_t)hf[(size_t)t * 3 + 2] * 3], h,
                                       &too_long);
        const int nr = C::rows_of(tr);
        for (int r = 0; r < nr; r++) {
            const int nj = C::row_candidates(tr, r, h);
            for (int j = 0; j < nj; j++, q++) {
                C::row_point(tr, r, j, h, &pos[(size_t)q * 3]);
                tri[(size_t)q] = t;
                cand[(size_t)q].q = q;
                C::cell_key(&pos[(size_t)q * 3], o, v, &cand[(size_t)q].cell, &cand[(size_t)q].key);
            }
        }
    }
    if (q != n_cands) { fprintf(stderr, "the passes disagree: %lld counted, %lld emitted\n", n_cands, (long long)q); return 4; }

    // the winners: a stable sort of the cells, then the head of every run walks its run
    std::stable_sort(cand.begin(), cand.end(), [](const Cand &x, const Cand &y) { return x.cell < y.cell; });
    std::vector<char> keep((size_t)n_cands, 0);
    for (size_t i = 0; i < cand.size();) {
        size_t best = i, j = i + 1;
        for (; j < cand.size() && cand[j].cell == cand[i].cell; j++)
            if (cand[j].key < cand[best].key || (cand[j].key == cand[best].key && cand[j].q < cand[best].q)) best = j;
        keep[(size_t)cand[best].q] = 1;
        i = j;
    }
    std::vector<float> out_p;
    std::vector<int32_t> out_t;
    for (int64_t i = 0; i < n_cands; i++)
        if (keep[(size_t)i]) {
            out_p.insert(out_p.end(), &pos[(size_t)i * 3], &pos[(size_t)i * 3] + 3);
            out_t.push_back(tri[(size_t)i]);
        }
    const int64_t m = (int64_t)out_t.size(), nc = n_cands;
    printf("triangles %d rows %lld candidates %lld kept %lld  origin %.9g %.9g %.9g\n", nf, n_rows, n_cands, (long long)m, (double)o[0], (double)o[1],
           (double)o[2]);
    f = fopen(argv[3], "wb");
    if (!f) { perror(argv[3]); return 2; }
    fwrite(&nc, 8, 1, f);
    fwrite(&m, 8, 1, f);
    fwrite(out_p.data(), 4, out_p.size(), f);
    fwrite(out_t.data(), 4, out_t.size(), f);
    fclose(f);
    return 0;
}
