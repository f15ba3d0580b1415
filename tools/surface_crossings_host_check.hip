// Host rehearsal of csrc/surface_crossings.hip: the statements of csrc/surface_crossings_shared.h (sc_face_box, sc_share_vertex, sc_pair
// with its division and square root) and the closed-box test of csrc/geom_shared.h (geom_boxes_meet) run serially on the CPU over every
// candidate in ascending (i, s, j, t) order.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off tools/surface_crossings_host_check.hip -o surface_crossings_host_check
//   surface_crossings_host_check BATCH.bin OUT.bin     (add -Xarch_host -fsanitize=address,undefined for a checked run)
//
// BATCH.bin: int32 B, V, F, flags (1 self | 2 between), has_group, P; B*V*3 float32; F*3 int32; B int32 (group, only when has_group);
//            F int32 (face_part) and P*P uint8 (part_skip), only when P > 0.
// OUT.bin:   int32 n; n*4 int32 (i, s, j, t); n int32 (events); n float32 (length): the crossing pairs.
// It does not cover the kernels' chunk order, tiles, LDS staging, scans, sort and atomics, nor the device's division and square root:
// those need the GPU tests.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>
#include "../psi-release_amd/csrc/surface_crossings_shared.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s BATCH.bin OUT.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[6];
    if (fread(hdr, 4, 6, f) != 6) return 2;
    const int B = hdr[0], V = hdr[1], F = hdr[2], flags = hdr[3], P = hdr[5];
    if (B < 1 || V < 1 || F < 1 || P < 0) { fprintf(stderr, "B, V and F are at least 1\n"); return 3; }
    std::vector<float> verts((size_t)B * V * 3);
    std::vector<int32_t> faces((size_t)F * 3), group((size_t)B, 0), part((size_t)F, 0);
    std::vector<uint8_t> skip((size_t)P * P, 0);
    if (fread(verts.data(), 4, verts.size(), f) != verts.size() || fread(faces.data(), 4, faces.size(), f) != faces.size()) return 2;
    if (hdr[4] && fread(group.data(), 4, group.size(), f) != group.size()) return 2;
    if (P && (fread(part.data(), 4, part.size(), f) != part.size() || fread(skip.data(), 1, skip.size(), f) != skip.size())) return 2;
    fclose(f);
    for (int32_t x : faces)
        if (x < 0 || x >= V) { fprintf(stderr, "face index %d outside [0, %d)\n", (int)x, V); return 3; }
    for (int32_t x : part)
        if (P && (x < 0 || x >= P)) { fprintf(stderr, "part %d outside [0, %d)\n", (int)x, P); return 3; }

    // triangles and face boxes of every (body, face)
    std::vector<float> tri((size_t)B * F * 9), lo((size_t)B * F * 3), hi((size_t)B * F * 3);
    for (int b = 0; b < B; b++)
        for (int s = 0; s < F; s++) {
            float p[3][3];
            for (int k = 0; k < 3; k++)
                for (int a = 0; a < 3; a++) p[k][a] = tri[((size_t)b * F + s) * 9 + k * 3 + a] = verts[((size_t)b * V + faces[(size_t)s * 3 + k]) * 3 + a];
            sc_face_box(p, &lo[((size_t)b * F + s) * 3], &hi[((size_t)b * F + s) * 3]);
        }

    std::vector<int32_t> pairs, events;
    std::vector<float> length;
    long long candidates = 0;
    for (int i = 0; i < B; i++)
        for (int s = 0; s < F; s++) {
            const size_t a = (size_t)i * F + s;
            const float(*p)[3] = (const float(*)[3]) & tri[a * 9];
            for (int j = i; j < B; j++) {
                if (i == j ? !(flags & SC_SELF) : (!(flags & SC_BETWEEN) || group[i] != group[j])) continue;
                for (int t = (i == j ? s + 1 : 0); t < F; t++) {
                    const size_t b = (size_t)j * F + t;
                    if (!geom_boxes_meet(&lo[a * 3], &hi[a * 3], &lo[b * 3], &hi[b * 3])) continue;
                    if (i == j) {
                        if (sc_share_vertex(&faces[(size_t)s * 3], &faces[(size_t)t * 3])) continue;
                        if (P && skip[(size_t)part[s] * P + part[t]]) continue;
                    }
                    candidates++;
                    float len;
                    const int ev = sc_pair(p, (const float(*)[3]) & tri[b * 9], &len);
                    if (ev == 0) continue;
                    const int32_t row[4] = {i, s, j, t};
                    pairs.insert(pairs.end(), row, row + 4);
                    events.push_back(ev);
                    length.push_back(len);
                }
            }
        }
    const int32_t n = (int32_t)events.size();
    printf("bodies %d vertices %d faces %d candidates %lld crossing pairs %d\n", B, V, F, candidates, (int)n);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    fwrite(&n, 4, 1, f);
    fwrite(pairs.data(), 4, pairs.size(), f);
    fwrite(events.data(), 4, events.size(), f);
    fwrite(length.data(), 4, length.size(), f);
    fclose(f);
    return 0;
}
