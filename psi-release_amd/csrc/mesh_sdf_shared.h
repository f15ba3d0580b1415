// What csrc/mesh_sdf.hip and csrc/mesh_winding.hip share: the node positions of a volume (one statement, so that both kernels see the same
// bits whatever contraction their file is compiled with), the checks of a node grid, and the winding side's view of a psi_mesh_sdf handle.
#pragma once
#include "psi_common.h"
#include <math.h>

#define MS_FN __host__ __device__ __forceinline__

// node i of an axis: gmin + (float)i * step, the product and the sum each rounded (the sampler's align_corners = True positions)
MS_FN float psi_mesh_node_pos(float gmin, float step, int i)
{
#pragma clang fp contract(off)
    return gmin + (float)i * step;
}

// The PSI_EINVAL rules of a node grid, and its spacing step[a] = (gmax[a] - gmin[a]) / (float)(D - 1).
static inline int psi_mesh_node_steps(const float gmin[3], const float gmax[3], int D, float step[3])
{
    PSI_REQUIRE(gmin && gmax, "null pointer");
    PSI_REQUIRE(D >= 2 && D <= 1024, "2 <= D <= 1024");
    for (int k = 0; k < 3; k++) {
        PSI_REQUIRE(std::isfinite(gmin[k]) && std::isfinite(gmax[k]), "the grid bounds must be finite");
        PSI_REQUIRE(gmax[k] > gmin[k], "gmax > gmin on every axis");
        step[k] = (gmax[k] - gmin[k]) / (float)(D - 1);
        PSI_REQUIRE(std::isfinite(step[k]) && step[k] > 0.0f, "the grid spacing must be a positive finite fp32 number");
    }
    return 0;
}

// The kept triangles of a handle on the host, [nk][3][3] fp32 (A, B, C in kept order), and the slot in which the winding side keeps what it
// builds from them at first use (psi_mesh_sdf_destroy calls `destroy` on it).
struct psi_mesh_aux {
    void *p;
    void (*destroy)(void *);
};
const float *psi_mesh_sdf_kept_tris(const psi_mesh_sdf *m, int *nk);
psi_mesh_aux *psi_mesh_sdf_aux(psi_mesh_sdf *m);
