// Host rehearsal of csrc/body_depth.hip: the statements of csrc/body_depth_shared.h and csrc/closest_point_shared.h (bd_record, bd_test,
// bd_key, bd_row, bd_grad_rows) run serially on the CPU in the kernels' order: per triple the slices of 2048 faces one after the other, in
// each the chunks of 256 faces in order, the smallest key per slice, then the smallest over the slices and the winner's statement once
// more; the aggregates added in triple order; the gradient rows sorted stably by target and every run added in order.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off tools/body_depth_host_check.hip -o body_depth_host_check
//   body_depth_host_check BATCH.bin OUT.bin            (add -Xarch_host -fsanitize=address,undefined for a checked run)
//
// BATCH.bin: int32 B, V, F, n, penalty, aggregates; B*V*3 float32; F*3 int32; n*3 int32 (i, j, v) ascending; B float32 (g).
// OUT.bin:   int32 n; n int32 (face); n int32 (region); n float32 (depth); n*3 float32 (r); n*3 float32 (bary); B*V*3 float32 (G); and
//            with aggregates != 0: B*B float32 (max_depth); B*B float64 (sum_depth); B*B float64 (sum_sq); B*V float32 (depth_of);
//            2*B float32 (loss).
// It does not cover the kernels' LDS staging, barriers and atomics, the chunk table, nor the device's division and square root: those need
// the GPU tests.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../psi-release_amd/csrc/body_depth_shared.h"

template <typename T>
static bool read_all(FILE *f, std::vector<T> &v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

template <typename T>
static void write_all(FILE *f, const std::vector<T> &v) { fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s BATCH.bin OUT.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[6];
    if (fread(hdr, 4, 6, f) != 6) return 2;
    const int B = hdr[0], V = hdr[1], F = hdr[2], n = hdr[3], penalty = hdr[4], aggregates = hdr[5];
    if (B < 1 || V < 1 || F < 1 || n < 0 || (penalty != BD_DEPTH && penalty != BD_SQUARED)) { fprintf(stderr, "bad header\n"); return 3; }
    std::vector<float> verts((size_t)B * V * 3), g((size_t)B);
    std::vector<int32_t> faces((size_t)F * 3), trip((size_t)n * 3);
    if (!read_all(f, verts) || !read_all(f, faces) || !read_all(f, trip) || !read_all(f, g)) return 2;
    fclose(f);
    for (int32_t x : faces)
        if (x < 0 || x >= V) { fprintf(stderr, "face index %d outside [0, %d)\n", (int)x, V); return 3; }
    for (int k = 0; k < n; k++) {
        const int32_t *t = &trip[(size_t)k * 3];
        if (t[0] < 0 || t[0] >= B || t[1] < 0 || t[1] >= B || t[0] == t[1] || t[2] < 0 || t[2] >= V) { fprintf(stderr, "triple %d\n", k); return 3; }
        if (k && !std::lexicographical_compare(t - 3, t, t, t + 3)) { fprintf(stderr, "triple %d is not above its predecessor\n", k); return 3; }
    }

    std::vector<BdRow> rows((size_t)n);
    const int n_slices = bd_slices(F);
    for (int k = 0; k < n; k++) {
        const int i = trip[(size_t)k * 3], j = trip[(size_t)k * 3 + 1], v = trip[(size_t)k * 3 + 2];
        const float *p = &verts[((size_t)i * V + v) * 3], *vj = &verts[(size_t)j * V * 3];
        unsigned long long best = ~0ull;
        for (int s = 0; s < n_slices; s++) {
            const int f_end = std::min(F, (s + 1) * BD_SLICE);
            unsigned long long in_slice = ~0ull;
            for (int f0 = s * BD_SLICE; f0 < f_end; f0 += BD_CHUNK)
                for (int t = f0; t < std::min(f_end, f0 + BD_CHUNK); t++) {
                    const BdRecord r = bd_record(vj, &faces[(size_t)t * 3]);
                    const unsigned long long key = bd_test(r.a[0], r.a[1], r.a[2], r.ab[0], r.ab[1], r.ab[2], r.ac[0], r.ac[1], r.ac[2], p[0], p[1], p[2], t);
                    in_slice = key < in_slice ? key : in_slice;
                }
            best = in_slice < best ? in_slice : best;
        }
        const int t = (int)(best & 0xffffffffull);
        rows[k] = bd_row(bd_record(vj, &faces[(size_t)t * 3]), p[0], p[1], p[2], t);
        if (bd_key(bd_d2(rows[k].r[0], rows[k].r[1], rows[k].r[2]), t) != best) { fprintf(stderr, "triple %d: the second run has other bits\n", k); return 4; }
    }

    // the gradient: four rows per triple, sorted stably by target, every run added in order
    std::vector<long long> targets((size_t)n * 4);
    std::vector<float> grow((size_t)n * 12), G((size_t)B * V * 3, 0.0f);
    for (int k = 0; k < n; k++) {
        const int i = trip[(size_t)k * 3], j = trip[(size_t)k * 3 + 1], v = trip[(size_t)k * 3 + 2];
        float out[4][3];
        bd_grad_rows(g[i], penalty, rows[k].depth, rows[k].r, rows[k].bary, out);
        targets[(size_t)k * 4] = (long long)i * V + v;
        for (int m = 0; m < 3; m++) targets[(size_t)k * 4 + 1 + m] = (long long)j * V + faces[(size_t)rows[k].face * 3 + m];
        for (int m = 0; m < 4; m++)
            for (int a = 0; a < 3; a++) grow[((size_t)k * 4 + m) * 3 + a] = out[m][a];
    }
    std::vector<size_t> order(targets.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return targets[a] < targets[b]; });
    for (size_t q = 0; q < order.size();) {
        const long long tgt = targets[order[q]];
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (; q < order.size() && targets[order[q]] == tgt; q++)
            for (int a = 0; a < 3; a++) acc[a] = acc[a] + grow[order[q] * 3 + a];
        for (int a = 0; a < 3; a++) G[(size_t)tgt * 3 + a] = acc[a];
    }

    std::vector<float> max_depth((size_t)B * B, 0.0f), depth_of((size_t)B * V, 0.0f), loss((size_t)2 * B, 0.0f);
    std::vector<double> sum_depth((size_t)B * B, 0.0), sum_sq((size_t)B * B, 0.0);
    if (aggregates) {
        for (int k = 0; k < n; k++) {
            const int i = trip[(size_t)k * 3], j = trip[(size_t)k * 3 + 1], v = trip[(size_t)k * 3 + 2];
            const float d = rows[k].depth;
            const double dd = (double)d;
            sum_depth[(size_t)i * B + j] += dd;
            sum_sq[(size_t)i * B + j] += dd * dd;
            if (bd_bits(d) > bd_bits(max_depth[(size_t)i * B + j])) max_depth[(size_t)i * B + j] = d;
            if (bd_bits(d) > bd_bits(depth_of[(size_t)i * V + v])) depth_of[(size_t)i * V + v] = d;
        }
        for (int i = 0; i < B; i++) {
            double total = 0.0, total_sq = 0.0;
            for (int j = 0; j < B; j++) {
                total += sum_depth[(size_t)i * B + j];
                total_sq += sum_sq[(size_t)i * B + j];
            }
            loss[i] = (float)total;
            loss[(size_t)B + i] = (float)total_sq;
        }
    }

    printf("bodies %d vertices %d faces %d slices %d triples %d\n", B, V, F, n_slices, n);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const int32_t n32 = n;
    fwrite(&n32, 4, 1, f);
    std::vector<int32_t> face((size_t)n), region((size_t)n);
    std::vector<float> depth((size_t)n), r((size_t)n * 3), bary((size_t)n * 3);
    for (int k = 0; k < n; k++) {
        face[k] = rows[k].face, region[k] = rows[k].region, depth[k] = rows[k].depth;
        for (int a = 0; a < 3; a++) r[(size_t)k * 3 + a] = rows[k].r[a], bary[(size_t)k * 3 + a] = rows[k].bary[a];
    }
    write_all(f, face), write_all(f, region), write_all(f, depth), write_all(f, r), write_all(f, bary), write_all(f, G);
    if (aggregates) write_all(f, max_depth), write_all(f, sum_depth), write_all(f, sum_sq), write_all(f, depth_of), write_all(f, loss);
    fclose(f);
    return 0;
}
