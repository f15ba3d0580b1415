// Host rehearsal of csrc/mesh_sdf.hip: the search of msdf_brick_kernel, brick by brick and batch by batch, run serially on the CPU with
// the very functions the kernel calls (closest point, shells, bounds, threshold), pruned against brute force, bit for bit.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off tools/mesh_sdf_host_check.hip -o mesh_sdf_host_check
//   mesh_sdf_host_check MESH.bin D gminx gminy gminz gmaxx gmaxy gmaxz OUT.f32     (add -fsanitize=address,undefined for a checked run)
//
// MESH.bin: int32 nv, int32 nf, nv*3 float32, nf*3 int32.  OUT.f32: the D^3 volume of the pruned search.  Exit status 1 when the two
// searches differ in any bit.  It does not cover the kernel's LDS staging, its scan or its barriers: those need the GPU tests.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include "../psi-release_amd/csrc/mesh_sdf.hip"

void psi_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}

static unsigned long long tests_done = 0;

static void brick(const HostMesh &hm, const NodeGrid &ng, int mode, int bx, int by, int bz, float *out)
{
    const int D = ng.D, nk = (int)hm.recs.size();
    unsigned long long best[BRICK][BRICK][BRICK];
    for (auto &a : best) for (auto &b : a) for (auto &c : b) c = ~0ull;
    auto live = [&](int x, int y, int z) { return bx + x < D && by + y < D && bz + z < D; };
    auto test = [&](int tri) {
        const TriRec &r = hm.recs[tri];
        for (int x = 0; x < BRICK; x++) for (int y = 0; y < BRICK; y++) for (int z = 0; z < BRICK; z++) {
            if (!live(x, y, z)) continue;
            float rx, ry, rz;
            closest_point(r.ab[0], r.ab[1], r.ab[2], r.ac[0], r.ac[1], r.ac[2], node_pos(ng, 0, bx + x) - r.a[0], node_pos(ng, 1, by + y) - r.a[1],
                          node_pos(ng, 2, bz + z) - r.a[2], rx, ry, rz);
            const unsigned long long k = key_of(dot3(rx, ry, rz, rx, ry, rz), r.idx);
            if (k < best[x][y][z]) best[x][y][z] = k;
            tests_done++;
        }
    };
    if (mode == 1) {
        for (int t = 0; t < nk; t++) test(t);
    } else {
        const CellGrid &cg = hm.cg;
        const Brick br = make_brick(ng, cg, bx, by, bz);
        const int smax = last_shell(cg, br);
        float thr2 = INFINITY;
        std::vector<char> seen(hm.cell_start.size() - 1, 0);
        for (int s = 0; s <= smax; s++) {
            if (s > 0) {
                const float lb = shell_bound(cg, br, s);
                if (lb > 0.0f && pruned(lb * lb, thr2)) break;
            }
            const Shell sh = shell_boxes(cg, br, s);
            const int ncell = sh.count();
            for (int base = 0; base < ncell; base += WG) {
                int total = 0;
                std::vector<int> kept;
                for (int i = base; i < std::min(ncell, base + WG); i++) {
                    int cx, cy, cz;
                    shell_cell(sh, i, cx, cy, cz);
                    if (cx < 0 || cy < 0 || cz < 0 || cx >= cg.n[0] || cy >= cg.n[1] || cz >= cg.n[2]) { fprintf(stderr, "cell outside the grid\n"); exit(2); }
                    const int cell = (cx * cg.n[1] + cy) * cg.n[2] + cz;
                    if (seen[cell]++) { fprintf(stderr, "cell visited twice\n"); exit(2); }
                    const int c = hm.cell_start[cell + 1] - hm.cell_start[cell];
                    if (c > 0 && !pruned(cell_gap2(cg, br, cx, cy, cz), thr2)) { kept.push_back(cell); total += c; }
                }
                for (int cell : kept)
                    for (int e = hm.cell_start[cell]; e < hm.cell_start[cell + 1]; e++) test(hm.bins[e]);
                if (total > 0) {
                    unsigned m = 0;
                    for (int x = 0; x < BRICK; x++) for (int y = 0; y < BRICK; y++) for (int z = 0; z < BRICK; z++)
                        if (live(x, y, z)) m = std::max(m, (unsigned)(best[x][y][z] >> 32));
                    float f;
                    memcpy(&f, &m, 4);
                    thr2 = prune_threshold2(f, ng.slack);
                }
            }
        }
    }
    for (int x = 0; x < BRICK; x++) for (int y = 0; y < BRICK; y++) for (int z = 0; z < BRICK; z++) {
        if (!live(x, y, z)) continue;
        const unsigned long long key = best[x][y][z];
        const int tri = (int)(unsigned)(key & 0xffffffffu);
        if (tri < 0 || tri >= nk) { fprintf(stderr, "a node found no triangle\n"); exit(2); }
        out[((size_t)(bx + x) * D + by + y) * D + bz + z] = signed_value(hm.recs[tri], hm.nrm[tri], (unsigned)(key >> 32), node_pos(ng, 0, bx + x),
                                                                           node_pos(ng, 1, by + y), node_pos(ng, 2, bz + z));
    }
}

int main(int argc, char **argv)
{
    if (argc != 10) { fprintf(stderr, "usage: %s MESH.bin D gmin[3] gmax[3] OUT.f32\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int nv = 0, nf = 0;
    if (fread(&nv, 4, 1, f) != 1 || fread(&nf, 4, 1, f) != 1) return 2;
    std::vector<float> hv((size_t)nv * 3);
    std::vector<int32_t> hf((size_t)nf * 3);
    if (fread(hv.data(), 4, hv.size(), f) != hv.size() || fread(hf.data(), 4, hf.size(), f) != hf.size()) return 2;
    fclose(f);
    HostMesh hm;
    if (build_host_mesh(hv, hf, nv, nf, hm) != 0) return 3;
    const int D = atoi(argv[2]);
    NodeGrid ng;
    float scale = hm.scale;
    for (int k = 0; k < 3; k++) {
        const float lo = (float)atof(argv[3 + k]), hi = (float)atof(argv[6 + k]);
        ng.gmin[k] = lo;
        ng.step[k] = (hi - lo) / (float)(D - 1);
        scale = fmaxf(scale, fmaxf(fabsf(lo), fabsf(hi)));
    }
    ng.D = D;
    ng.slack = REL_SLACK * scale;
    printf("kept %d dropped %d welded %d open_edges %d  cells %d x %d x %d  bin entries %zu\n", hm.info[0], hm.info[1], hm.info[2], hm.info[3],
           hm.cg.n[0], hm.cg.n[1], hm.cg.n[2], hm.bins.size());
    std::vector<float> a((size_t)D * D * D), b((size_t)D * D * D);
    unsigned long long n[2];
    for (int mode = 0; mode < 2; mode++) {
        tests_done = 0;
        for (int bx = 0; bx < D; bx += BRICK) for (int by = 0; by < D; by += BRICK) for (int bz = 0; bz < D; bz += BRICK)
            brick(hm, ng, mode, bx, by, bz, mode ? b.data() : a.data());
        n[mode] = tests_done;
    }
    size_t diff = 0;
    for (size_t i = 0; i < a.size(); i++) diff += memcmp(&a[i], &b[i], 4) != 0;
    printf("pair tests: pruned %llu, brute %llu (%.2f %%); nodes that differ: %zu\n", n[0], n[1], 100.0 * n[0] / n[1], diff);
    f = fopen(argv[9], "wb");
    if (!f) { perror(argv[9]); return 2; }
    fwrite(a.data(), 4, a.size(), f);
    fclose(f);
    return diff ? 1 : 0;
}
