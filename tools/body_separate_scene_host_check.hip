// Host rehearsal of the scene kernel of csrc/body_separate.hip: the scene statements of csrc/body_separate_shared.h (bs_scene_of,
// bs_scene_box, bs_scene_vertex, bs_torque) run serially on the CPU in the kernel's order.  Per body and chunk of 256 vertices: the sample
// and G of every vertex, the eight fp64 terms of the vertices in the scene, the 256-lane tree.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off tools/body_separate_scene_host_check.hip -o body_separate_scene_host_check
//   body_separate_scene_host_check BATCH.bin OUT.bin      (add -Xarch_host -fsanitize=address,undefined for a checked run)
//
// BATCH.bin: int32 B, V, D, S, has_id; float32 w_scene; B*V*3 float32 (verts); B*3 float32 (p); S*D*D*D float32 (sdf); S*3 float32 (gmin);
//            S*3 float32 (gmax); B int32 (scene_id) when has_id.
// OUT.bin:   B*nchunk*6 float64 (chunks), B*nchunk int32 (count), B*nchunk float64 (loss), B*V float32 (sdf), B*V*3 float32 (G).
// It does not cover the kernel's indexing of the grid, the LDS and lane-shift form of the tree, nor the device's fp64 division: those need
// the GPU tests.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>
#include "../psi-release_amd/csrc/body_separate_shared.h"

template <typename T>
static bool read_all(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

template <typename T>
static void write_all(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

static bs3 load3(const float *p) { return bs_make(p[0], p[1], p[2]); }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s BATCH.bin OUT.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[5];
    float w_scene;
    if (fread(hdr, 4, 5, f) != 5 || fread(&w_scene, 4, 1, f) != 1) return 2;
    const int B = hdr[0], V = hdr[1], D = hdr[2], S = hdr[3], has_id = hdr[4];
    if (B < 1 || V < 1 || D < 2 || D > 512 || S < 1 || S > 64 || (long long)B * V > (1ll << 26)) { fprintf(stderr, "bad header\n"); return 3; }
    const int nchunk = (V + BS_CHUNK - 1) / BS_CHUNK;
    const size_t vol = (size_t)D * D * D;
    std::vector<float> verts((size_t)B * V * 3), p((size_t)B * 3), sdf((size_t)S * vol), gmin((size_t)S * 3), gmax((size_t)S * 3);
    std::vector<int32_t> scene_id(has_id ? (size_t)B : 0);
    if (!read_all(f, verts) || !read_all(f, p) || !read_all(f, sdf) || !read_all(f, gmin) || !read_all(f, gmax) || !read_all(f, scene_id)) return 2;
    fclose(f);

    std::vector<double> chunks((size_t)B * nchunk * 6), loss((size_t)B * nchunk);
    std::vector<int32_t> count((size_t)B * nchunk);
    std::vector<float> value((size_t)B * V), G((size_t)B * V * 3);
    for (int b = 0; b < B; b++) {
        const int sc = bs_scene_of(has_id ? scene_id.data() : nullptr, b, S);
        const BsSceneBox box = bs_scene_box(&gmin[3 * sc], &gmax[3 * sc], D);
        for (int ch = 0; ch < nchunk; ch++) {
            double lane[BS_CHUNK][8];
            for (int l = 0; l < BS_CHUNK; l++) {
                const int v = ch * BS_CHUNK + l;
                for (int a = 0; a < 8; a++) lane[l][a] = 0.0;
                if (v >= V) continue;
                const size_t at = ((size_t)b * V + v) * 3;
                const bs3 x = load3(&verts[at]);
                bs3 g;
                bool inside;
                const BsSceneSample sm = bs_scene_vertex(&sdf[sc * vol], D, box, x, w_scene, g, inside);
                if (inside) {
                    const bs3 cr = bs_torque(x, load3(&p[3 * b]), g);
                    lane[l][0] = (double)g.x, lane[l][1] = (double)g.y, lane[l][2] = (double)g.z;
                    lane[l][3] = (double)cr.x, lane[l][4] = (double)cr.y, lane[l][5] = (double)cr.z;
                    lane[l][6] = (double)(-sm.value), lane[l][7] = 1.0;
                }
                value[(size_t)b * V + v] = sm.value;
                G[at] = g.x, G[at + 1] = g.y, G[at + 2] = g.z;
            }
            for (int stride = BS_CHUNK / 2; stride >= 1; stride /= 2)
                for (int l = 0; l < stride; l++)
                    for (int a = 0; a < 8; a++) lane[l][a] = lane[l][a] + lane[l + stride][a];
            const size_t c = (size_t)b * nchunk + ch;
            for (int a = 0; a < 6; a++) chunks[c * 6 + a] = lane[0][a];
            loss[c] = lane[0][6];
            count[c] = (int32_t)lane[0][7];
        }
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    write_all(f, chunks), write_all(f, count), write_all(f, loss), write_all(f, value), write_all(f, G);
    fclose(f);
    printf("bodies %d vertices %d chunks %d scenes %d of %d^3\n", B, V, nchunk, S, D);
    return 0;
}
