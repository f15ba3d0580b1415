// Host rehearsal of csrc/mesh_winding.hip: the per-pair, per-dipole and per-cluster statements of mwind_brick_kernel (geom_half_omega
// of csrc/geom_shared.h, half_dipole, mwind_far, brick_box, the host-side clustering) run serially on the CPU, brick by brick, in the
// kernel's order of summation (fp32 within a chunk of 256 records, fp64 across chunks).  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/mesh_winding_host_check.hip -o mesh_winding_host_check
//   mesh_winding_host_check MESH.bin D gminx gminy gminz gmaxx gmaxy gmaxz BETA CLUSTER OUT.f32   (add -fsanitize=address,undefined for a checked run)
//
// MESH.bin: int32 nv, int32 nf, nv*3 float32, nf*3 int32.  OUT.f32: the D^3 volume of f.  Prints the kept triangles, the clusters and the
// (node, triangle) and (node, dipole) tests.  It does not cover the kernel's LDS staging, its scan or its barriers, nor the device's
// arctangent, division, square root and contraction: those need the GPU tests.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include "../psi-release_amd/csrc/mesh_sdf.hip"
#include "../psi-release_amd/csrc/mesh_winding.hip"

void psi_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}

namespace W = psi_mwind;

struct Staged {
    W::WRec r;
    bool dipole;
};

int main(int argc, char **argv)
{
    if (argc != 12) { fprintf(stderr, "usage: %s MESH.bin D gmin[3] gmax[3] BETA CLUSTER OUT.f32\n", argv[0]); return 2; }
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
    const int nk = hm.info[0];
    const int D = atoi(argv[2]);
    const float beta = (float)atof(argv[9]);
    const int cluster = atoi(argv[10]);
    float gmin[3], gmax[3];
    for (int k = 0; k < 3; k++) {
        gmin[k] = (float)atof(argv[3 + k]);
        gmax[k] = (float)atof(argv[6 + k]);
    }
    W::Nodes ng;
    if (psi_mesh_node_steps(gmin, gmax, D, ng.step) != 0) return 3;
    if (!(beta >= 0.0f) || !std::isfinite(beta) || cluster < W::MIN_CLUSTER || cluster > W::MAX_CLUSTER) { fprintf(stderr, "beta or cluster refused\n"); return 3; }
    for (int k = 0; k < 3; k++) ng.gmin[k] = gmin[k];
    ng.D = D;

    std::vector<W::WRec> recs;
    std::vector<W::CRec> clus;
    if (beta == 0.0f) W::kept_records(hm.kept.data(), nk, recs);
    else W::build_clusters(hm.kept.data(), nk, cluster, recs, clus);
    const int nc = (int)clus.size();

    std::vector<float> out((size_t)D * D * D);
    unsigned long long n_tri = 0, n_dip = 0;
    std::vector<Staged> list;
    std::vector<size_t> batch;     // where the records of each batch of 256 clusters begin: the kernel's chunks restart there
    for (int bx = 0; bx < D; bx += W::BRICK) for (int by = 0; by < D; by += W::BRICK) for (int bz = 0; bz < D; bz += W::BRICK) {
        // the brick's records in the kernel's order
        list.clear();
        batch.assign(1, 0);
        if (beta == 0.0f) {
            for (int t = 0; t < nk; t++) list.push_back(Staged{recs[t], false});
        } else {
            float lo[3], hi[3];
            W::brick_box(ng, bx, by, bz, lo, hi);
            for (int j = 0; j < nc; j++) {
                if (j > 0 && j % W::WG == 0) batch.push_back(list.size());
                if (W::mwind_far(clus[j].c, clus[j].r, lo, hi, beta)) {
                    W::WRec d;
                    memset(&d, 0, sizeof(d));
                    for (int k = 0; k < 3; k++) { d.a[k] = clus[j].c[k]; d.b[k] = clus[j].n[k]; }
                    list.push_back(Staged{d, true});
                } else {
                    for (int t = j * cluster; t < std::min(nk, (j + 1) * cluster); t++) list.push_back(Staged{recs[t], false});
                }
            }
        }
        batch.push_back(list.size());
        const int x1 = std::min(D, bx + W::BRICK), y1 = std::min(D, by + W::BRICK), z1 = std::min(D, bz + W::BRICK);
        const unsigned long long nlive = (unsigned long long)(x1 - bx) * (y1 - by) * (z1 - bz);
        for (const Staged &s : list) (s.dipole ? n_dip : n_tri) += nlive;
        for (int ix = bx; ix < x1; ix++) for (int iy = by; iy < y1; iy++) for (int iz = bz; iz < z1; iz++) {
            const float px = psi_mesh_node_pos(ng.gmin[0], ng.step[0], ix), py = psi_mesh_node_pos(ng.gmin[1], ng.step[1], iy),
                        pz = psi_mesh_node_pos(ng.gmin[2], ng.step[2], iz);
            double acc = 0.0;
            for (size_t b = 0; b + 1 < batch.size(); b++)
            for (size_t i = batch[b]; i < batch[b + 1];) {
                float s = 0.0f;
                const size_t end = std::min(batch[b + 1], i + (size_t)W::WG);
                while (i < end) {
                    const W::WRec &r = list[i].r;
                    s += list[i].dipole ? W::half_dipole(r.a[0], r.a[1], r.a[2], r.b[0], r.b[1], r.b[2], px, py, pz)
                                        : geom_half_omega(r.a[0], r.a[1], r.a[2], r.b[0], r.b[1], r.b[2], r.c[0], r.c[1], r.c[2], r.n[0], r.n[1], r.n[2],
                                                          px, py, pz);
                    i++;
                }
                acc += (double)s;
            }
            out[((size_t)ix * D + iy) * D + iz] = W::f_of_sum(acc);
        }
    }
    printf("kept %d clusters %d of %d  beta %g  triangle tests %llu dipole tests %llu\n", nk, nc, cluster, (double)beta, n_tri, n_dip);
    f = fopen(argv[11], "wb");
    if (!f) { perror(argv[11]); return 2; }
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}
