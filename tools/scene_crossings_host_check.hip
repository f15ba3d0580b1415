// Host rehearsal of csrc/scene_crossings.hip: the candidate rule (sc_face_box, geom_boxes_meet), sc_pair with its division and square
// root, the key and the un-key of csrc/scene_crossings_shared.h run serially on the CPU over every (body face, scene triangle), and the
// host half of psi_scene_crossings_create (scn_build: Morton order, records, chunk boxes, scene box).  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off tools/scene_crossings_host_check.hip -o scene_crossings_host_check
//   scene_crossings_host_check BATCH.bin OUT.bin       (add -Xarch_host -fsanitize=address,undefined for a checked run)
//   scene_crossings_host_check --keys                  (the key round-trips at the limits; exit status 1 at the first failure)
//
// BATCH.bin: int32 B, V, F, nv, nf; B*V*3 float32; F*3 int32; nv*3 float32; nf*3 int32.
// OUT.bin:   int32 n, nf, nK; n*3 int32 (i, s, t) sorted by key; n int32 (events); n float32 (length); nf int32 (order); nK*6 float32
//            (chunk boxes); 6 float32 (scene box).  The rows are produced from the builder's records in chunk order, keyed, sorted and
//            un-keyed, as the kernels do.
// It does not cover the kernels' tiles, LDS staging, scans and atomics, nor the device's division and square root: those need the GPU tests.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>
#include "../psi-release_amd/csrc/scene_crossings_shared.h"

static int check_keys()
{
    // (B, F, nf) at the limits: the largest body and face against the largest triangle index, products just below 2^63
    const long long cases[][3] = {{1, 1, 1}, {4, 352, 528}, {46340, (1 << 21) - 1, 94908256}, {1, 1, 0x7fffffffll}, {46340, 1, 0x7fffffffll},
                                  {32, 20904, 197000}, {2, (1 << 21) - 1, 0x7fffffffll}};
    for (const auto &c : cases) {
        const long long B = c[0], F = c[1], nf = c[2];
        if (!scn_key_fits(B, F, nf)) { printf("FAILED: %lld %lld %lld does not fit\n", B, F, nf); return 1; }
        const long long is[] = {0, B / 2, B - 1}, ss[] = {0, F / 2, F - 1}, ts[] = {0, nf / 2, nf - 1};
        long long last = -1, li = -1, ls = -1, lt = -1;     // the key ascends wherever (i, s, t) does
        for (long long i : is)
            for (long long s : ss)
                for (long long t : ts) {
                    const long long key = scn_key((int)i, (int)s, (int)t, (int)F, (int)nf);
                    int r[3];
                    scn_unkey(key, (int)F, (int)nf, r);
                    if (key < 0 || r[0] != i || r[1] != s || r[2] != t) { printf("FAILED: (%lld,%lld,%lld) of (%lld,%lld,%lld) -> %lld\n", i, s, t, B, F, nf, key); return 1; }
                    const bool above = i > li || (i == li && (s > ls || (s == ls && t > lt)));
                    if (above && key <= last) { printf("FAILED: keys do not ascend with (i, s, t)\n"); return 1; }
                    if (above) last = key, li = i, ls = s, lt = t;
                }
    }
    // one past the limit is refused
    if (scn_key_fits(46340, (1 << 21) - 1, 94908257) || scn_key_fits(3037000500ll, 3037000500ll, 1) || scn_key_fits(0, 1, 1)) {
        printf("FAILED: a product of 2^63 or more fits\n");
        return 1;
    }
    printf("keys round-trip at the limits\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "--keys")) return check_keys();
    if (argc != 3) { fprintf(stderr, "usage: %s BATCH.bin OUT.bin | --keys\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[5];
    if (fread(hdr, 4, 5, f) != 5) return 2;
    const int B = hdr[0], V = hdr[1], F = hdr[2], nv = hdr[3], nf = hdr[4];
    if (B < 1 || V < 1 || F < 1 || nv < 1 || nf < 1) { fprintf(stderr, "B, V, F, nv and nf are at least 1\n"); return 3; }
    std::vector<float> verts((size_t)B * V * 3), sverts((size_t)nv * 3);
    std::vector<int32_t> faces((size_t)F * 3), sfaces((size_t)nf * 3);
    if (fread(verts.data(), 4, verts.size(), f) != verts.size() || fread(faces.data(), 4, faces.size(), f) != faces.size() ||
        fread(sverts.data(), 4, sverts.size(), f) != sverts.size() || fread(sfaces.data(), 4, sfaces.size(), f) != sfaces.size())
        return 2;
    fclose(f);
    for (int32_t x : faces)
        if (x < 0 || x >= V) { fprintf(stderr, "face index %d outside [0, %d)\n", (int)x, V); return 3; }
    if (!scn_key_fits(B, F, nf)) { fprintf(stderr, "B F nf does not fit the key\n"); return 3; }

    ScnBuilt hb;
    long long bad = -1;
    const int rc = scn_build(sverts.data(), nv, sfaces.data(), nf, &hb, &bad);
    if (rc) { fprintf(stderr, "scn_build refuses the scene: code %d at triangle %lld\n", rc, bad); return 3; }
    const int nK = (int)(hb.chunk_boxes.size() / 6);

    // every body face against every record, in chunk order: the unsorted list the emit pass writes
    struct Row { long long key; int32_t ev; float len; };
    std::vector<Row> rows;
    long long candidates = 0;
    for (int i = 0; i < B; i++)
        for (int s = 0; s < F; s++) {
            float p[3][3], alo[3], ahi[3];
            for (int k = 0; k < 3; k++)
                for (int a = 0; a < 3; a++) p[k][a] = verts[((size_t)i * V + faces[(size_t)s * 3 + k]) * 3 + a];
            sc_face_box(p, alo, ahi);
            for (int pos = 0; pos < nf; pos++) {
                const float *r = &hb.recs[(size_t)pos * SCN_REC_ROWS * 4];
                const float q[3][3] = {{r[0], r[1], r[2]}, {r[3], r[4], r[5]}, {r[6], r[7], r[8]}};
                float blo[3], bhi[3];
                sc_face_box(q, blo, bhi);
                if (!geom_boxes_meet(alo, ahi, blo, bhi)) continue;
                candidates++;
                float len;
                const int ev = sc_pair(p, q, &len);
                if (ev == 0) continue;
                int32_t t;
                memcpy(&t, r + 9, sizeof(t));
                rows.push_back({scn_key(i, s, t, F, nf), ev, len});
            }
        }
    std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) { return a.key < b.key; });
    const int32_t n = (int32_t)rows.size();
    std::vector<int32_t> pairs((size_t)n * 3), events((size_t)n);
    std::vector<float> length((size_t)n);
    for (int32_t c = 0; c < n; c++) {
        int r[3];
        scn_unkey(rows[c].key, F, nf, r);
        for (int a = 0; a < 3; a++) pairs[(size_t)c * 3 + a] = r[a];
        events[c] = rows[c].ev;
        length[c] = rows[c].len;
    }
    printf("bodies %d vertices %d faces %d scene triangles %d chunks %d candidates %lld crossing pairs %d\n", B, V, F, nf, nK, candidates, (int)n);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const int32_t head[3] = {n, nf, nK};
    fwrite(head, 4, 3, f);
    fwrite(pairs.data(), 4, pairs.size(), f);
    fwrite(events.data(), 4, events.size(), f);
    fwrite(length.data(), 4, length.size(), f);
    fwrite(hb.order.data(), 4, hb.order.size(), f);
    fwrite(hb.chunk_boxes.data(), 4, hb.chunk_boxes.size(), f);
    fwrite(hb.box, 4, 6, f);
    fclose(f);
    return 0;
}
