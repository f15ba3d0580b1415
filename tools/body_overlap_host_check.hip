// Host rehearsal of csrc/body_overlap.hip: the per-triple statements of csrc/geom_shared.h (geom_in_box, geom_boxes_meet, geom_normal,
// geom_half_omega) and csrc/body_overlap_shared.h (bo_w_of_sum, bo_inside) run serially on the CPU in the kernels' order: pairs
// ascending, vertices ascending, fp32 within a chunk of 256 faces, the chunk sums in fp64 within a slice of 2048 faces, the slice sums in
// fp64 in slice order.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/body_overlap_host_check.hip -o body_overlap_host_check
//   body_overlap_host_check BATCH.bin OUT.bin          (add -Xarch_host -fsanitize=address,undefined for a checked run)
//
// BATCH.bin: int32 B, V, F, has_group; B*V*3 float32; F*3 int32; B int32 (group, read only when has_group).
// OUT.bin:   int32 n; n*3 int32 (i, j, v); n float32 (w); B*B int32 (counts); B*V uint8 (inside).
// It does not cover the kernels' LDS staging, ballots, scans, barriers and atomics, nor the device's arctangent, division, square root and
// contraction: those need the GPU tests.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../psi-release_amd/csrc/body_overlap_shared.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s BATCH.bin OUT.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[4];
    if (fread(hdr, 4, 4, f) != 4) return 2;
    const int B = hdr[0], V = hdr[1], F = hdr[2];
    if (B < 1 || V < 1 || F < 1) { fprintf(stderr, "B, V and F are at least 1\n"); return 3; }
    std::vector<float> verts((size_t)B * V * 3);
    std::vector<int32_t> faces((size_t)F * 3), group((size_t)B, 0);
    if (fread(verts.data(), 4, verts.size(), f) != verts.size() || fread(faces.data(), 4, faces.size(), f) != faces.size()) return 2;
    if (hdr[3] && fread(group.data(), 4, group.size(), f) != group.size()) return 2;
    fclose(f);
    for (int32_t x : faces)
        if (x < 0 || x >= V) { fprintf(stderr, "face index %d outside [0, %d)\n", (int)x, V); return 3; }

    std::vector<float> lo((size_t)B * 3), hi((size_t)B * 3);
    for (int b = 0; b < B; b++)
        for (int a = 0; a < 3; a++) {
            float mn = INFINITY, mx = -INFINITY;
            for (int v = 0; v < V; v++) {
                const float x = verts[((size_t)b * V + v) * 3 + a];
                mn = fminf(mn, x);
                mx = fmaxf(mx, x);
            }
            lo[(size_t)b * 3 + a] = mn;
            hi[(size_t)b * 3 + a] = mx;
        }

    std::vector<int32_t> cand, counts((size_t)B * B, 0);
    std::vector<float> w;
    std::vector<uint8_t> inside((size_t)B * V, 0);
    const int n_slices = bo_slices(F);
    for (int i = 0; i < B; i++)
        for (int j = 0; j < B; j++) {
            if (i == j || group[i] != group[j]) continue;
            if (!geom_boxes_meet(&lo[(size_t)i * 3], &hi[(size_t)i * 3], &lo[(size_t)j * 3], &hi[(size_t)j * 3])) continue;
            const float *vj = &verts[(size_t)j * V * 3];
            for (int v = 0; v < V; v++) {
                const float *p = &verts[((size_t)i * V + v) * 3];
                if (!geom_in_box(p[0], p[1], p[2], &lo[(size_t)j * 3], &hi[(size_t)j * 3])) continue;
                double total = 0.0;
                for (int s = 0; s < n_slices; s++) {
                    const int f_end = std::min(F, (s + 1) * BO_SLICE);
                    double acc = 0.0;
                    for (int f0 = s * BO_SLICE; f0 < f_end; f0 += BO_CHUNK) {
                        float sum = 0.0f;
                        for (int t = f0; t < std::min(f_end, f0 + BO_CHUNK); t++) {
                            const float *A = vj + (size_t)faces[(size_t)t * 3] * 3, *Bv = vj + (size_t)faces[(size_t)t * 3 + 1] * 3,
                                        *C = vj + (size_t)faces[(size_t)t * 3 + 2] * 3;
                            float n[3];
                            geom_normal(A, Bv, C, n);
                            sum += geom_half_omega(A[0], A[1], A[2], Bv[0], Bv[1], Bv[2], C[0], C[1], C[2], n[0], n[1], n[2], p[0], p[1], p[2]);
                        }
                        acc += (double)sum;
                    }
                    total += acc;
                }
                const float wv = bo_w_of_sum(total);
                cand.push_back(i);
                cand.push_back(j);
                cand.push_back(v);
                w.push_back(wv);
                if (bo_inside(wv)) {
                    counts[(size_t)i * B + j]++;
                    inside[(size_t)i * V + v] = 1;
                }
            }
        }
    const int32_t n = (int32_t)w.size();
    printf("bodies %d vertices %d faces %d slices %d candidates %d\n", B, V, F, n_slices, (int)n);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    fwrite(&n, 4, 1, f);
    fwrite(cand.data(), 4, cand.size(), f);
    fwrite(w.data(), 4, w.size(), f);
    fwrite(counts.data(), 4, counts.size(), f);
    fwrite(inside.data(), 1, inside.size(), f);
    fclose(f);
    return 0;
}
