// Host rehearsal of csrc/raster_bodies.hip: the result images of a small scene rendered serially on the CPU with the very functions the
// kernels call (raster_device.h's setup, coverage and depth statements; vertex_normal, setup_body_face, compose_pixel).  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off tools/result_images_host_check.hip -o result_images_host_check
//   result_images_host_check IN.bin OUT.bin                                   (add -fsanitize=address,undefined for a checked run)
//
// IN.bin:  int32 nsv, nsf, has_rgb, B, V, F, M, n, W, H; float32 near, bg[3]; then scene verts [nsv,3] f32, scene faces [nsf,3] i32 (nsf = 0: no
//          scene), vrgb [nsv,3] f32 when has_rgb, bverts [B,V,3] f32, bfaces [F,3] i32, draw_body [M] i32, draw_view [M] i32, draw_rgb [M,3] f32,
//          w2c [n,12] f32, intr [n,4] f32.
// OUT.bin: rgb [n,H,W,3] u8, depth [n,H,W] f32, draw i32, body_depth f32, body_id i32, counts [M,2] i32, normals [B,V,3] f32, voff [V+1] i32,
//          vface [3F] i32.
// It does not cover the binning, the LDS z-buffer, the passes or the wave-level count: those need the GPU tests.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../psi-release_amd/csrc/raster_bodies.hip"

void psi_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}

void *psi_scratch(size_t, hipStream_t) { return nullptr; }

template <typename T>
static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

// every pixel of the piece's box against the key image of its view
static void draw_record(const PieceRec &r, int W, int H, unsigned long long *keys)
{
    int x0, y0, x1, y1;
    if (!pixel_box(r.U0, r.V0, r.U1, r.V1, r.U2, r.V2, W, H, x0, y0, x1, y1)) return;
    for (int y = y0; y <= y1; y++)
        for (int x = x0; x <= x1; x++) {
            unsigned long long key;
            if (pixel_key(r, x, y, key)) keys[(size_t)y * W + x] = key_min(keys[(size_t)y * W + x], key);
        }
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN.bin OUT.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int> hd = take<int>(f, 10);
    const int nsv = hd[0], nsf = hd[1], has_rgb = hd[2], B = hd[3], V = hd[4], F = hd[5], M = hd[6], n = hd[7], W = hd[8], H = hd[9];
    const std::vector<float> fl = take<float>(f, 4);
    const float near_ = fl[0], bg[3] = {fl[1], fl[2], fl[3]};
    std::vector<float> sverts = take<float>(f, (size_t)nsv * 3);
    std::vector<int> sfaces = take<int>(f, (size_t)nsf * 3);
    std::vector<float> vrgb = take<float>(f, has_rgb ? (size_t)nsv * 3 : 0);
    std::vector<float> bverts = take<float>(f, (size_t)B * V * 3);
    std::vector<int> bfaces = take<int>(f, (size_t)F * 3);
    std::vector<int> draw_body = take<int>(f, M), draw_view = take<int>(f, M);
    std::vector<float> draw_rgb = take<float>(f, (size_t)M * 3), w2c = take<float>(f, (size_t)n * 12), intr = take<float>(f, (size_t)n * 4);
    fclose(f);
    if ((long long)M * F >= (1LL << 31)) return 3;
    for (int i : sfaces) if (i < 0 || i >= nsv) return 3;
    for (int d = 0; d < M; d++) if (draw_body[d] < 0 || draw_body[d] >= B || draw_view[d] < 0 || draw_view[d] >= n) return 3;

    psi_raster_bodies tp = {};
    std::vector<int> voff, vface;
    if (!vertex_face_lists(bfaces, V, F, voff, vface)) return 3;
    tp.faces = bfaces.data();
    tp.voff = voff.data();
    tp.vface = vface.data();
    tp.V = V;
    tp.F = F;

    const size_t npix = (size_t)n * W * H;
    std::vector<float> normals((size_t)B * V * 3);
    for (int b = 0; b < B; b++)
        for (int v = 0; v < V; v++) vertex_normal(bverts.data() + (size_t)b * V * 3, tp, v, &normals[((size_t)b * V + v) * 3]);

    // the scene's snapshot: depth and triangle index per pixel
    std::vector<unsigned long long> skeys(npix, ~0ull), bkeys(npix, ~0ull);
    for (int view = 0; view < n; view++) {
        const View vw = load_view(w2c.data(), intr.data(), view);
        for (int t = 0; t < nsf; t++) {
            CamVertT<1> v[3];
            for (int k = 0; k < 3; k++) {
                v[k] = to_camera<1>(vw, sverts.data() + (size_t)sfaces[(size_t)t * 3 + k] * 3);
                v[k].a[0] = 0.0f;
            }
            PieceT<1> pc[2];
            int dropped = 0;
            const int np = setup_triangle(vw, near_, v[0], v[1], v[2], pc, &dropped);
            for (int k = 0; k < np; k++) {
                PieceRec r;
                if (piece_record(pc[k], t, W, H, r) != NOBOX) draw_record(r, W, H, skeys.data() + (size_t)view * W * H);
            }
        }
    }
    std::vector<float> sdepth(npix, 0.0f);
    std::vector<int> stri(npix, -1);
    for (size_t o = 0; o < npix; o++)
        if (skeys[o] != ~0ull) {
            const unsigned zb = (unsigned)(skeys[o] >> 32);
            memcpy(&sdepth[o], &zb, 4);
            stri[o] = (int)(unsigned)(skeys[o] & 0xffffffffu);
        }
    // the bodies' key image
    for (int d = 0; d < M; d++) {
        const int view = draw_view[d];
        const View vw = load_view(w2c.data(), intr.data(), view);
        for (int face = 0; face < F; face++) {
            PieceRec r[2];
            unsigned box[2];
            setup_body_face(tp, bverts.data() + (size_t)draw_body[d] * V * 3, vw, near_, W, H, d, face, r, box);
            for (int k = 0; k < 2; k++)
                if (box[k] != NOBOX) draw_record(r[k], W, H, bkeys.data() + (size_t)view * W * H);
        }
    }
    // compose
    Scene sc = {};
    if (nsf) {
        sc.mesh.verts = sverts.data();
        sc.mesh.faces = sfaces.data();
        sc.mesh.nv = nsv;
        sc.mesh.nf = nsf;
        sc.vrgb = has_rgb ? vrgb.data() : nullptr;
        sc.depth = sdepth.data();
        sc.tri = stri.data();
    }
    const Draws dr = {draw_body.data(), draw_view.data(), draw_rgb.data(), bverts.data()};
    std::vector<unsigned char> rgb(npix * 3);
    std::vector<float> depth(npix), bdepth(npix);
    std::vector<int> draw(npix), bid(npix), counts((size_t)M * 2, 0);
    for (int view = 0; view < n; view++) {
        const View vw = load_view(w2c.data(), intr.data(), view);
        for (int py = 0; py < H; py++)
            for (int px = 0; px < W; px++) {
                const size_t o = ((size_t)view * H + py) * W + px;
                const PixelOut p = compose_pixel(sc, tp, dr, vw, near_, px, py, o, bkeys[o], bg);
                memcpy(&rgb[o * 3], p.rgb, 3);
                depth[o] = p.depth;
                draw[o] = p.draw;
                bdepth[o] = p.bdepth;
                bid[o] = p.bid;
                if (p.draw_of >= 0) {
                    counts[(size_t)p.draw_of * 2 + 0]++;
                    if (p.visible) counts[(size_t)p.draw_of * 2 + 1]++;
                }
            }
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    fwrite(rgb.data(), 1, rgb.size(), f);
    fwrite(depth.data(), 4, npix, f);
    fwrite(draw.data(), 4, npix, f);
    fwrite(bdepth.data(), 4, npix, f);
    fwrite(bid.data(), 4, npix, f);
    fwrite(counts.data(), 4, counts.size(), f);
    fwrite(normals.data(), 4, normals.size(), f);
    fwrite(voff.data(), 4, voff.size(), f);
    fwrite(vface.data(), 4, vface.size(), f);
    fclose(f);
    return 0;
}
