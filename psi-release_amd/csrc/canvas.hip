// psi_snapshot_canvas: the CVAE's input images of n rendered views in one call.
//
// What the reference does per image on the host (utils_prox_snapshots_virtualcam.py data_preprocessing :266-330, is_body_occluded :342-378;
// batch_gen_hdf5.py:398-439): clip, scale to [-1, 1] by the view's maximum, bilinear resize into a centred canvas, and the mean depth of a
// window around the body's pixel against the body's own depth.  Here for every view and both modalities at once:
//
//   canvas_max_kernel    one read of every pixel.  A workgroup reduces min(x, clip) over its 4096 pixels and sends ONE integer atomicMax on
//                        the bit pattern (values are >= 0, so the order of the bits is the order of the floats) to the view's slot; a NaN
//                        sets the view's flag with an integer atomicOr.  Both are order-independent: the maximum is exact and the call is
//                        bit-identical from run to run and whatever other views it holds.  No floating-point atomics.
//   canvas_write_kernel  one thread per canvas pixel: four gathers, each scaled (2 c) / max - 1, then the interpolation in PyTorch's
//                        association.  The first workgroup of a view also sums the window (fp64, row-major, one adder) and writes the
//                        view's max_d, seg_max and usable.
//
// Compiled with -ffp-contract=off: the statements of section 12 are evaluated as written, product by product; the one fused multiply-add
// of the contract (the source index) is written as one.
#include "psi_common.h"

namespace psi_canvas {

constexpr int WG = 256;
constexpr int PIX_PER_WG = 4096;     // canvas_max_kernel: 4 float4 per thread

struct Slot {                        // per view, zeroed by the call
    unsigned max_bits[2];            // depth, seg: bits of max over the view of min(x, clip), NaN pixels left out
    unsigned nan_flags;              // bit 0: depth holds a NaN, bit 1: seg does
    unsigned pad;
};

__device__ __forceinline__ void take(float x, float clip, float &m, bool &nan)
{
    nan |= x != x;
    const float c = x < clip ? x : clip;      // NaN compares false -> clip; the flag above zeroes the view anyway
    m = (x == x && c > m) ? c : m;
}

template <bool VEC>
__global__ __launch_bounds__(WG) void canvas_max_kernel(const float *__restrict__ depth, const float *__restrict__ seg, long HW, int nb,
                                                        float clip_d, float clip_s, Slot *__restrict__ slots)
{
    const int mod = blockIdx.y;
    const long view = blockIdx.x / nb;
    const long b = blockIdx.x % nb;
    const float *src = (mod ? seg : depth) + (size_t)view * (size_t)HW;
    const float clip = mod ? clip_s : clip_d;
    const long lo = b * PIX_PER_WG;
    const long hi = lo + PIX_PER_WG < HW ? lo + PIX_PER_WG : HW;
    float m = 0.0f;
    bool nan = false;
    if (VEC) {      // HW % 4 == 0 and a 16-byte aligned base: every view starts on a float4
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const long i4 = lo / 4 + k * WG + threadIdx.x;
            v[k] = i4 * 4 < hi ? s4[i4] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            take(v[k].x, clip, m, nan);
            take(v[k].y, clip, m, nan);
            take(v[k].z, clip, m, nan);
            take(v[k].w, clip, m, nan);
        }
    } else {
        for (long i = lo + threadIdx.x; i < hi; i += WG) take(src[i], clip, m, nan);
    }
    // m >= 0 and not NaN: its bits order like the value
    unsigned bits = __float_as_uint(m);
    unsigned flag = nan ? 1u : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned ob = __shfl_xor(bits, off);
        const unsigned of = __shfl_xor(flag, off);
        bits = ob > bits ? ob : bits;
        flag |= of;
    }
    __shared__ unsigned s_bits[WG / PSI_WAVE], s_flag[WG / PSI_WAVE];
    const int wave = threadIdx.x / PSI_WAVE;
    if ((threadIdx.x & (PSI_WAVE - 1)) == 0) {
        s_bits[wave] = bits;
        s_flag[wave] = flag;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < WG / PSI_WAVE; w++) {
            bits = s_bits[w] > bits ? s_bits[w] : bits;
            flag |= s_flag[w];
        }
        if (bits) atomicMax(&slots[view].max_bits[mod], bits);
        if (flag) atomicOr(&slots[view].nan_flags, 1u << mod);
    }
}

// one tap of the scaled image: (2 c) / max - 1 in the reference's order
__device__ __forceinline__ float tap(const float *__restrict__ src, long idx, float clip, float mx)
{
    const float x = src[idx];
    const float c = x < clip ? x : clip;
    return (2.0f * c) / mx - 1.0f;
}

// source index and weights of F.interpolate(mode='bilinear', align_corners=False): scale = float(in) / out.  scale (dst + 0.5) - 0.5 is ONE
// fused multiply-add, as PyTorch's own kernels evaluate it (CPU builds with FMA, and the GPU ones): at a scale that is no power of two the
// twice-rounded form moves src by an ulp, i.e. a weight by up to 2^-17 at src ~ 100 — far above the canvas tolerance
__device__ __forceinline__ void source(int dst, float scale, int in, int &i0, int &i1, float &l0, float &l1)
{
    float s = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
    s = s < 0.0f ? 0.0f : s;
    i0 = (int)s;
    i0 = i0 < in - 1 ? i0 : in - 1;      // cannot bind for s < in (a guard for the address, not a rule of the contract)
    i1 = i0 + 1 < in - 1 ? i0 + 1 : in - 1;
    l1 = s - (float)i0;
    l0 = 1.0f - l1;
}

struct Place {      // where the resized image sits in the canvas
    int th, tw;     // canvas
    int oh, ow;     // resized image
    int y0, x0;     // its first canvas row / column
};

__global__ __launch_bounds__(WG) void canvas_write_kernel(const float *__restrict__ depth, const float *__restrict__ seg, int H, int W, Place pl,
                                                          int nb, float clip_d, float clip_s, const int *__restrict__ windows,
                                                          const float *__restrict__ target_z, const Slot *__restrict__ slots,
                                                          float *__restrict__ depth_canvas, float *__restrict__ seg_canvas,
                                                          float *__restrict__ max_d, float *__restrict__ seg_max, int *__restrict__ usable)
{
    const int mod = blockIdx.y;
    const long view = blockIdx.x / nb;
    const int b = blockIdx.x % nb;
    const size_t HW = (size_t)H * (size_t)W;
    const Slot sl = slots[view];
    const float mxd = __uint_as_float(sl.max_bits[0]), mxs = __uint_as_float(sl.max_bits[1]);
    const bool good = mxd > 0.0f && mxs > 0.0f && sl.nan_flags == 0;

    const int p = b * WG + threadIdx.x;
    if (p < pl.th * pl.tw) {
        const int py = p / pl.tw, px = p % pl.tw;
        const int oy = py - pl.y0, ox = px - pl.x0;
        float out = 0.0f;
        if (good && oy >= 0 && oy < pl.oh && ox >= 0 && ox < pl.ow) {
            const float *src = (mod ? seg : depth) + view * HW;
            const float clip = mod ? clip_s : clip_d;
            const float mx = mod ? mxs : mxd;
            int y0, y1, x0, x1;
            float l0y, l1y, l0x, l1x;
            source(oy, (float)H / (float)pl.oh, H, y0, y1, l0y, l1y);
            source(ox, (float)W / (float)pl.ow, W, x0, x1, l0x, l1x);
            const float a = tap(src, (long)y0 * W + x0, clip, mx), bb = tap(src, (long)y0 * W + x1, clip, mx);
            const float c = tap(src, (long)y1 * W + x0, clip, mx), d = tap(src, (long)y1 * W + x1, clip, mx);
            out = l0y * (l0x * a + l1x * bb) + l1y * (l0x * c + l1x * d);
        }
        (mod ? seg_canvas : depth_canvas)[(size_t)view * pl.th * pl.tw + p] = out;
    }

    if (b != 0 || mod != 0) return;       // the view's scalars: its first workgroup (uniform per workgroup, so the barriers below are safe)
    bool ok = good;
    if (good && windows) {
        int wx0 = windows[view * 4 + 0], wy0 = windows[view * 4 + 1], wx1 = windows[view * 4 + 2], wy1 = windows[view * 4 + 3];
        wx0 = wx0 < 0 ? 0 : wx0;
        wy0 = wy0 < 0 ? 0 : wy0;
        wx1 = wx1 > W ? W : wx1;
        wy1 = wy1 > H ? H : wy1;
        const int ww = wx1 > wx0 ? wx1 - wx0 : 0, wh = wy1 > wy0 ? wy1 - wy0 : 0;
        const long count = (long)ww * wh;
        const float *src = depth + view * HW;
        __shared__ double s_val[WG];
        double sum = 0.0;
        for (long base = 0; base < count; base += WG) {      // row-major, one adder: the order is part of the contract
            const long k = base + threadIdx.x;
            if (k < count) s_val[threadIdx.x] = (double)src[(wy0 + k / ww) * (long)W + wx0 + k % ww];
            __syncthreads();
            if (threadIdx.x == 0) {
                const int lim = count - base < WG ? (int)(count - base) : WG;
                for (int j = 0; j < lim; j++) sum += s_val[j];
            }
            __syncthreads();
        }
        ok = count > 0 && sum / (double)count > (double)target_z[view];
    }
    if (threadIdx.x == 0) {
        max_d[view] = mxd;
        seg_max[view] = mxs;
        usable[view] = ok ? 1 : 0;
    }
}

}   // namespace psi_canvas

extern "C" size_t psi_snapshot_canvas_workspace_bytes(int n_views)
{
    return n_views > 0 ? (size_t)n_views * sizeof(psi_canvas::Slot) : 0;
}

extern "C" int psi_snapshot_canvas(const float *d_depth, const float *d_seg, int n_views, int H, int W, int th, int tw, float clip_depth,
                                   float clip_seg, const int32_t *d_windows, const float *d_target_z, float *d_depth_canvas,
                                   float *d_seg_canvas, float *d_max_d, float *d_seg_max, int32_t *d_usable, void *d_workspace, void *stream)
{
    using namespace psi_canvas;
    PSI_REQUIRE(d_depth && d_seg && d_depth_canvas && d_seg_canvas && d_max_d && d_seg_max && d_usable, "null pointer");
    PSI_REQUIRE((d_windows == nullptr) == (d_target_z == nullptr), "windows and target depths come together");
    PSI_REQUIRE(n_views >= 1 && H >= 1 && W >= 1, "n_views, H, W >= 1");
    PSI_REQUIRE((long)H * W < (1l << 31), "H * W < 2^31");
    PSI_REQUIRE(th >= 2 && tw >= 2 && th % 2 == 0 && tw % 2 == 0 && (long)th * tw < (1l << 31), "th, tw even and >= 2");
    PSI_REQUIRE(clip_depth > 0.0f && clip_seg > 0.0f, "clips > 0");
    Place pl;
    pl.th = th;
    pl.tw = tw;
    if (H >= W) {       // batch_gen_hdf5.py:398-439: factor = th / H, the width rounded down to an even number, centred
        pl.oh = th;
        pl.ow = (int)((double)W * ((double)th / (double)H)) / 2 * 2;
        pl.y0 = 0;
        pl.x0 = tw / 2 - pl.ow / 2;
    } else {
        pl.ow = tw;
        pl.oh = (int)(((double)tw / (double)W) * (double)H) / 2 * 2;
        pl.x0 = 0;
        pl.y0 = th / 2 - pl.oh / 2;
    }
    PSI_REQUIRE(pl.oh >= 2 && pl.ow >= 2 && pl.oh <= th && pl.ow <= tw, "the resized image is empty or does not fit the canvas");
    const long HW = (long)H * W;
    const int nb_max = psi_cdiv(HW, PIX_PER_WG), nb_px = psi_cdiv((long)th * tw, WG);
    PSI_REQUIRE((long)n_views * nb_max < (1l << 31) && (long)n_views * nb_px < (1l << 31), "n_views * workgroups per view < 2^31");
    hipStream_t st = (hipStream_t)stream;
    Slot *slots = (Slot *)(d_workspace ? d_workspace : psi_scratch(psi_snapshot_canvas_workspace_bytes(n_views), st));
    if (!slots) {
        psi_set_error("psi_snapshot_canvas: no workspace");
        return PSI_ENOMEM;
    }
    PSI_CHECK_HIP(hipMemsetAsync(slots, 0, psi_snapshot_canvas_workspace_bytes(n_views), st));
    const bool vec = HW % 4 == 0 && (((uintptr_t)d_depth | (uintptr_t)d_seg) & 15) == 0;
    const dim3 g1((unsigned)((long)n_views * nb_max), 2);
    if (vec)
        hipLaunchKernelGGL(canvas_max_kernel<true>, g1, dim3(WG), 0, st, d_depth, d_seg, HW, nb_max, clip_depth, clip_seg, slots);
    else
        hipLaunchKernelGGL(canvas_max_kernel<false>, g1, dim3(WG), 0, st, d_depth, d_seg, HW, nb_max, clip_depth, clip_seg, slots);
    PSI_CHECK_LAUNCH("canvas_max_kernel");
    hipLaunchKernelGGL(canvas_write_kernel, dim3((unsigned)((long)n_views * nb_px), 2), dim3(WG), 0, st, d_depth, d_seg, H, W, pl, nb_px,
                       clip_depth, clip_seg, d_windows, d_target_z, slots, d_depth_canvas, d_seg_canvas, d_max_d, d_seg_max, d_usable);
    PSI_CHECK_LAUNCH("canvas_write_kernel");
    return 0;
}
