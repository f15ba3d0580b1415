// Where the kinematic chain of the pose stage runs in the fused fitting engine (fit.hip), as a function without dependencies that the
// engine's decisions go through; tools/chain_plan_host_check.hip walks every body of every plan on the host.
//
// The head kernel needs of the pose stage only what blend_fwd reads — the feature row.  The chain behind it (G, A: psi_pose_fwd_links,
// lbs_device.h) is first read two launches later, so it can ride in the launch between: blend_fwd_h_kernel<.., LINKS = true> (lbs.hip)
// carries n_links_wg workgroups behind its stream workgroups, wave w of links workgroup g running the bodies
//     (4 g + w) bodies_per_wave + t,    t = 0 .. bodies_per_wave - 1    (those below B)
// one after the other.  That is free only while the role stays in the stream's shadow, so it is ON when all of these hold, and otherwise
// the chain stays in the head kernel:
//   * the head kernels run as clusters (hc > 1): with one workgroup per body the head launch fills the chip with bodies and the chain is not
//     what it waits for;
//   * blend_fwd's grid is one row (grid_y == 1, B <= 64): the role's block ids are "behind the stream's" in x only;
//   * n_links_wg <= PSI_CHAIN_WG_MAX = 8: one links workgroup per XCD (blocks are dealt round-robin over the 8 XCDs), each on a CU the
//     stream leaves free;
//   * n_links_wg <= cus - n_stream: EVERY workgroup of the launch is resident at once (the stream runs one workgroup per CU).  A links
//     workgroup that queued behind a 12 us stream workgroup would lengthen the launch instead.
// bodies_per_wave = ceil(B / 32): 1 up to B = 32 (8 workgroups x 4 waves), 2 up to 64.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSI_CHAIN_HD __host__ __device__
#else
#define PSI_CHAIN_HD
#endif

constexpr int PSI_CHAIN_WG_MAX = 8;
constexpr int PSI_CHAIN_WAVES = 4;        // waves of a links workgroup (blend_fwd's 256 threads)

struct PsiChainPlan {
    int n_links_wg;               // 0: off — the chain runs in the head kernel
    int bodies_per_wave;
};

// B >= 1 bodies, hc = workgroups per body of the head kernels, n_stream x grid_y = blend_fwd's stream grid, cus = compute units of the device
PSI_CHAIN_HD inline PsiChainPlan psi_chain_plan(int B, int hc, int n_stream, int grid_y, int cus)
{
    const PsiChainPlan off = {0, 0};
    if (B < 1 || hc <= 1 || grid_y != 1) return off;
    PsiChainPlan p;
    p.bodies_per_wave = (B + 31) / 32;
    const int per_wg = PSI_CHAIN_WAVES * p.bodies_per_wave;
    p.n_links_wg = (B + per_wg - 1) / per_wg;
    if (p.n_links_wg > PSI_CHAIN_WG_MAX || p.n_links_wg > cus - n_stream) return off;
    return p;
}

// first body of wave w of links workgroup g (the wave takes this one and the next bodies_per_wave - 1, as far as they are below B)
PSI_CHAIN_HD inline int psi_chain_first_body(const PsiChainPlan &p, int g, int w) { return (g * PSI_CHAIN_WAVES + w) * p.bodies_per_wave; }
