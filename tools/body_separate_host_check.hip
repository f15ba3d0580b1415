// Host rehearsal of csrc/body_separate.hip: the statements of csrc/body_separate_shared.h (bs_rotation, bs_pose, bs_torque, bs_adam,
// bs_quat_step) run serially on the CPU in the kernels' order.  Per step k = 1 .. n: the pose of every vertex under the current state, the
// six wrench terms of every vertex for that step's G, the 256-lane tree of every chunk in fp64, the chunks added in order and rounded once,
// the Adam step and the quaternion update.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off tools/body_separate_host_check.hip -o body_separate_host_check
//   body_separate_host_check BATCH.bin OUT.bin            (add -Xarch_host -fsanitize=address,undefined for a checked run)
//
// BATCH.bin: int32 B, V, n, has_fixed; float64 lr_t, lr_r, b1, b2, eps; B*V*3 float32 (base); B*3 float32 (pivot); B*4 (quat), B*3
//            (transl), B*6 (m), B*6 (s) float32; B int32 (fixed) when has_fixed; n*B*V*3 float32 (G of every step).
// OUT.bin:   per step: B*V*3 float32 (verts), B*nchunk*6 float64 (chunks), B*6 float32 (g6), then the state after the step: B*4 (quat),
//            B*3 (transl), B*6 (m), B*6 (s) float32.
// It does not cover the kernels' indexing, the LDS and lane-shift form of the tree, nor the device's division and square root: those need
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
    int32_t hdr[4];
    double par[5];
    if (fread(hdr, 4, 4, f) != 4 || fread(par, 8, 5, f) != 5) return 2;
    const int B = hdr[0], V = hdr[1], n = hdr[2], has_fixed = hdr[3];
    if (B < 1 || V < 1 || n < 0 || (long long)B * V > (1ll << 26)) { fprintf(stderr, "bad header\n"); return 3; }
    const int nchunk = (V + BS_CHUNK - 1) / BS_CHUNK;
    std::vector<float> base((size_t)B * V * 3), pivot((size_t)B * 3), quat((size_t)B * 4), transl((size_t)B * 3), m((size_t)B * 6), s((size_t)B * 6);
    std::vector<int32_t> fixed(has_fixed ? (size_t)B : 0);
    std::vector<float> G((size_t)n * B * V * 3);
    if (!read_all(f, base) || !read_all(f, pivot) || !read_all(f, quat) || !read_all(f, transl) || !read_all(f, m) || !read_all(f, s) ||
        !read_all(f, fixed) || !read_all(f, G))
        return 2;
    fclose(f);

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    std::vector<float> verts((size_t)B * V * 3), g6((size_t)B * 6);
    std::vector<double> chunks((size_t)B * nchunk * 6);
    for (int k = 1; k <= n; k++) {
        const float *Gk = &G[(size_t)(k - 1) * B * V * 3];
        BsStep K;
        K.b1 = (float)par[2], K.b2 = (float)par[3], K.eps = (float)par[4], K.lr_t = (float)par[0], K.lr_r = (float)par[1];
        K.c1 = (float)(1.0 - pow(par[2], (double)k)), K.c2 = (float)(1.0 - pow(par[3], (double)k));
        for (int b = 0; b < B; b++) {
            BsQuat q;
            q.w = quat[4 * b], q.x = quat[4 * b + 1], q.y = quat[4 * b + 2], q.z = quat[4 * b + 3];
            const bs3 t = load3(&transl[3 * b]), c = load3(&pivot[3 * b]);
            const BsRot R = bs_rotation(q);
            const bs3 p = bs_centre(c, t);
            const bool same = bs_is_identity(q, t);
            for (int v = 0; v < V; v++) {
                const size_t at = ((size_t)b * V + v) * 3;
                const bs3 x = bs_pose(load3(&base[at]), R, c, p, same);
                verts[at] = x.x, verts[at + 1] = x.y, verts[at + 2] = x.z;
            }
            for (int ch = 0; ch < nchunk; ch++) {
                double lane[BS_CHUNK][6];
                for (int l = 0; l < BS_CHUNK; l++) {
                    const int v = ch * BS_CHUNK + l;
                    for (int a = 0; a < 6; a++) lane[l][a] = 0.0;
                    if (v >= V) continue;
                    const size_t at = ((size_t)b * V + v) * 3;
                    const bs3 g = load3(Gk + at);
                    const bs3 cr = bs_torque(load3(&verts[at]), p, g);
                    lane[l][0] = (double)g.x, lane[l][1] = (double)g.y, lane[l][2] = (double)g.z;
                    lane[l][3] = (double)cr.x, lane[l][4] = (double)cr.y, lane[l][5] = (double)cr.z;
                }
                for (int stride = BS_CHUNK / 2; stride >= 1; stride /= 2)
                    for (int l = 0; l < stride; l++)
                        for (int a = 0; a < 6; a++) lane[l][a] = lane[l][a] + lane[l + stride][a];
                for (int a = 0; a < 6; a++) chunks[((size_t)b * nchunk + ch) * 6 + a] = lane[0][a];
            }
            float u[6];
            for (int a = 0; a < 6; a++) {
                double acc = 0.0;
                for (int ch = 0; ch < nchunk; ch++) acc = acc + chunks[((size_t)b * nchunk + ch) * 6 + a];
                g6[(size_t)b * 6 + a] = (float)acc;
                const float g = (has_fixed && fixed[b] != 0) ? 0.0f : g6[(size_t)b * 6 + a];
                u[a] = bs_adam(m[(size_t)b * 6 + a], s[(size_t)b * 6 + a], g, K);
            }
            for (int a = 0; a < 3; a++) transl[3 * b + a] = transl[3 * b + a] - K.lr_t * u[a];
            q = bs_quat_step(q, bs_make(-(K.lr_r * u[3]), -(K.lr_r * u[4]), -(K.lr_r * u[5])));
            quat[4 * b] = q.w, quat[4 * b + 1] = q.x, quat[4 * b + 2] = q.y, quat[4 * b + 3] = q.z;
        }
        write_all(f, verts), write_all(f, chunks), write_all(f, g6), write_all(f, quat), write_all(f, transl), write_all(f, m), write_all(f, s);
    }
    fclose(f);
    printf("bodies %d vertices %d chunks %d steps %d\n", B, V, nchunk, n);
    return 0;
}
