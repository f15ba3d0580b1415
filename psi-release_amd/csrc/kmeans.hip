// k-means in the protocol of scipy.cluster.vq.kmeans, for gfx950 — replaces, in the reference's diversity evaluation,
//   codes, dist = scipy.cluster.vq.kmeans(body_param_list, 20);  vecs, dist = scipy.cluster.vq.vq(body_param_list, codes)
//                                                                              utils/utils_eval_diversity.py:93-95
// One restart is scipy's _kmeans statement for statement:
//   prev = +inf;  repeat { code, dist = vq(obs, book);  avg = mean(dist);  book = centroids of the members, codes without members
//   REMOVED (order of the others kept);  diff = |prev - avg|;  prev = avg } until not (diff > thresh)
// and all R restarts advance together: the restart is a grid dimension of every launch, so 20 restarts x N points fill the chip where
// one restart of N = 5000 would not.  One Lloyd iteration = three launches:
//   km_assign   (N / 256, R)   nearest code of every point (first minimum wins), per-workgroup fp64 partial of sum(dist)
//   km_update   (P, k, R)      per code and point slice: fp64 sum of the member rows, member count
//   km_finalize (R)            partials combined in workgroup order -> new book (compacted), avg, the convergence decision
// Arithmetic: squared distance sum_f (x_f - c_f)^2 in fp32, features in index order (one fma per feature); dist = sqrtf; sums, counts
// and avg in fp64 / integers, combined in a fixed order: no floating-point atomics, bit-identical from run to run and independent of
// how the iterations are split into psi_kmeans_iterate calls.  A converged restart is frozen: its workgroups return at once.
#include "psi_common.h"
#include "blob.h"
#include <math.h>
#include <vector>

typedef float km_f4 __attribute__((ext_vector_type(4)));

struct psi_kmeans {
    const float *obs;     // [N][d], borrowed
    int N, d, k, R;
    float thresh;
    int P, CH, NWA;       // update slices (of 256 * CH points), assign workgroups
    char *blob;
    float *obsT;          // [d][N]: the assign kernel's loads are coalesced over the points
    float *book;          // [R][k][d], first k_eff[r] rows valid
    int *k_eff, *iters, *conv;     // [R]
    double *prev, *avg;   // [R]
    int *code;            // [R][N]
    double *psum;         // [R][P][k][d]
    int *pcnt;            // [R][P][k]
    double *pdist;        // [R][NWA]
};

namespace {

constexpr int KB = 256;

// TR: x is [d][N] (transposed copy), else [N][d].  book: restart r's rows at book + r * bstride; k_eff / conv nullable (k rows, not converged).
template <int KC, bool TR>
__global__ __launch_bounds__(KB) void km_assign_kernel(const float *__restrict__ x, int N, int d, const float *__restrict__ book, size_t bstride,
                                                       const int *__restrict__ k_eff, int k, const int *__restrict__ conv,
                                                       int *__restrict__ code, float *__restrict__ dist, double *__restrict__ pdist)
{
    const int r = blockIdx.y, t = threadIdx.x;
    if (conv && conv[r]) return;
    const int ke = k_eff ? k_eff[r] : k;
    extern __shared__ float sb[];                                  // [d][KC]: the codes of one feature are adjacent (16-byte broadcast reads)
    const float *bk = book + (size_t)r * bstride;
    for (int idx = t; idx < d * KC; idx += KB) {
        const int f = idx / KC, c = idx % KC;
        sb[idx] = c < ke ? bk[(size_t)c * d + f] : 0.0f;
    }
    __syncthreads();
    const int i = blockIdx.x * KB + t;
    const bool live = i < N;
    const size_t ii = live ? i : N - 1;
    float acc[KC];
#pragma unroll
    for (int c = 0; c < KC; c++) acc[c] = 0.0f;
    for (int f = 0; f < d; f++) {
        const float xf = TR ? x[(size_t)f * N + ii] : x[ii * d + f];
        const float *row = sb + f * KC;
#pragma unroll
        for (int c = 0; c < KC; c += 4) {
            if (c < ke) {                                           // uniform: whole groups of removed codes cost nothing
                const km_f4 cb = *(const km_f4 *)(row + c);
                float df = xf - cb.x;
                acc[c] = __builtin_fmaf(df, df, acc[c]);
                df = xf - cb.y;
                acc[c + 1] = __builtin_fmaf(df, df, acc[c + 1]);
                df = xf - cb.z;
                acc[c + 2] = __builtin_fmaf(df, df, acc[c + 2]);
                df = xf - cb.w;
                acc[c + 3] = __builtin_fmaf(df, df, acc[c + 3]);
            }
        }
    }
    float best = acc[0];
    int bc = 0;
#pragma unroll
    for (int c = 1; c < KC; c++)
        if (c < ke && acc[c] < best) {                              // strict: the FIRST minimum wins (scipy's vq)
            best = acc[c];
            bc = c;
        }
    const float ds = sqrtf(best);
    if (live) {
        code[(size_t)r * N + i] = bc;
        if (dist) dist[(size_t)r * N + i] = ds;
    }
    if (!pdist) return;
    double s = live ? (double)ds : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);    // fixed tree
    __shared__ double red[KB / 64];
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
        double a = red[0];
#pragma unroll
        for (int w = 1; w < KB / 64; w++) a += red[w];
        pdist[(size_t)r * gridDim.x + blockIdx.x] = a;
    }
}

// members of code c in slice p, in point order: an ordered compaction of 256 labels at a time (ballot + popcount), then the member rows
// are summed by G groups of feature lanes, group g taking list entries g, g + G, ... — a fixed order per (slice, code, feature)
__global__ __launch_bounds__(KB) void km_update_kernel(psi_kmeans km)
{
    const int p = blockIdx.x, c = blockIdx.y, r = blockIdx.z, t = threadIdx.x;
    if (km.conv[r] || c >= km.k_eff[r]) return;
    const int N = km.N, d = km.d;
    const int DP = d <= 64 ? 64 : 128, G = KB / DP, f = t & (DP - 1), g = t / DP;
    __shared__ int list[KB];
    __shared__ int wcnt[KB / 64];
    __shared__ double red[KB / 64][128];
    const int *lab = km.code + (size_t)r * N;
    double s = 0.0;
    int cnt = 0;
    for (int ch = 0; ch < km.CH; ch++) {
        const long i = ((long)p * km.CH + ch) * KB + t;
        const bool mem = i < N && lab[i] == c;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(mem);
        const int lane = t & 63, w = t >> 6;
        if (lane == 0) wcnt[w] = (int)__builtin_popcountll(bal);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int q = 0; q < KB / 64; q++) {
            off += q < w ? wcnt[q] : 0;
            total += wcnt[q];
        }
        if (mem) list[off + (int)__builtin_popcountll(bal & ((1ull << lane) - 1ull))] = (int)i;
        __syncthreads();
        if (f < d)
            for (int e = g; e < total; e += G) s += (double)km.obs[(size_t)list[e] * d + f];
        cnt += total;
        __syncthreads();                                            // list / wcnt are rewritten by the next chunk
    }
    red[g][f & 127] = s;
    __syncthreads();
    if (g == 0 && f < d) {
        double a = red[0][f];
        for (int q = 1; q < G; q++) a += red[q][f];
        km.psum[(((size_t)r * km.P + p) * km.k + c) * d + f] = a;
    }
    if (t == 0) km.pcnt[((size_t)r * km.P + p) * km.k + c] = cnt;
}

__global__ __launch_bounds__(KB) void km_finalize_kernel(psi_kmeans km)
{
    const int r = blockIdx.x, t = threadIdx.x;
    if (km.conv[r]) return;
    const int ke = km.k_eff[r], d = km.d, k = km.k, P = km.P;
    __shared__ int cnt[64], nidx[64];
    __shared__ int newke;
    if (t < ke) {
        int a = 0;
        for (int p = 0; p < P; p++) a += km.pcnt[((size_t)r * P + p) * k + t];
        cnt[t] = a;
    }
    __syncthreads();
    if (t == 0) {
        int j = 0;
        for (int c = 0; c < ke; c++) nidx[c] = cnt[c] > 0 ? j++ : -1;     // codes without members are removed, the order of the others kept
        newke = j;
    }
    __syncthreads();
    for (int idx = t; idx < ke * d; idx += KB) {
        const int c = idx / d, f = idx % d;
        if (nidx[c] < 0) continue;
        double s = 0.0;
        for (int p = 0; p < P; p++) s += km.psum[(((size_t)r * P + p) * k + c) * d + f];    // slice order
        km.book[((size_t)r * k + nidx[c]) * d + f] = (float)(s / (double)cnt[c]);
    }
    if (t == 0) {
        double a = 0.0;
        for (int w = 0; w < km.NWA; w++) a += km.pdist[(size_t)r * km.NWA + w];              // workgroup order
        a /= (double)km.N;
        const double diff = fabs(km.prev[r] - a);                   // inf on the first iteration
        km.prev[r] = a;
        km.avg[r] = a;
        km.iters[r] += 1;
        km.k_eff[r] = newke;
        if (!(diff > (double)km.thresh)) km.conv[r] = 1;
    }
}

__global__ __launch_bounds__(KB) void km_transpose_kernel(const float *__restrict__ obs, long n, int N, int d, float *__restrict__ obsT)
{
    const long idx = (long)blockIdx.x * KB + threadIdx.x;
    if (idx >= n) return;
    const long i = idx / d;
    const int f = (int)(idx % d);
    obsT[(size_t)f * N + i] = obs[idx];
}

__global__ __launch_bounds__(64) void km_init_kernel(psi_kmeans km)
{
    const int r = threadIdx.x;
    if (r >= km.R) return;
    km.k_eff[r] = km.k;
    km.iters[r] = 0;
    km.conv[r] = 0;
    km.prev[r] = (double)INFINITY;
    km.avg[r] = (double)INFINITY;
}

template <bool TR>
int km_launch_assign(const float *x, int N, int d, const float *book, size_t bstride, const int *k_eff, int k, const int *conv, int R,
                     int *code, float *dist, double *pdist, hipStream_t st)
{
    const dim3 grid(psi_cdiv(N, KB), R);
#define PSI_KM_ASSIGN(KC_)                                                                                                          \
    hipLaunchKernelGGL((km_assign_kernel<KC_, TR>), grid, dim3(KB), (size_t)d * KC_ * sizeof(float), st, x, N, d, book, bstride, k_eff, k, \
                       conv, code, dist, pdist)
    if (k <= 8) PSI_KM_ASSIGN(8);
    else if (k <= 16) PSI_KM_ASSIGN(16);
    else if (k <= 24) PSI_KM_ASSIGN(24);
    else if (k <= 32) PSI_KM_ASSIGN(32);
    else if (k <= 48) PSI_KM_ASSIGN(48);
    else PSI_KM_ASSIGN(64);
#undef PSI_KM_ASSIGN
    PSI_CHECK_LAUNCH("km_assign_kernel");
    return 0;
}

}  // namespace

extern "C" int psi_kmeans_create(psi_kmeans **out, const float *obs, int N, int d, const float *guess, int k, int R, float thresh)
{
    PSI_REQUIRE(out && obs && guess, "null pointer");
    PSI_REQUIRE(d >= 1 && d <= 128 && k >= 1 && k <= 64 && R >= 1 && R <= 64, "d <= 128, k <= 64, R <= 64");
    PSI_REQUIRE(N >= k && (long)N * d < (1L << 31), "N >= k");
    // a one-off on the default stream, between two device synchronisations: obs / guess may have been produced on any stream
    PSI_CHECK_HIP(hipDeviceSynchronize());
    psi_kmeans *km = new psi_kmeans();
    km->obs = obs;
    km->N = N; km->d = d; km->k = k; km->R = R;
    km->thresh = thresh;
    km->CH = psi_cdiv(psi_cdiv(N, 64), KB);                          // at most 64 slices
    km->P = psi_cdiv(N, (long)KB * km->CH);
    km->NWA = psi_cdiv(N, KB);
    const size_t Rz = (size_t)R;
    PsiBlob T;                                                   // all but the codebook start uninitialised: the two kernels below write them
    T.raw(km->obsT, (size_t)N * d * 4);
    T.copy(km->book, guess, Rz * k * d * 4);
    T.raw(km->k_eff, Rz * 4);
    T.raw(km->iters, Rz * 4);
    T.raw(km->conv, Rz * 4);
    T.raw(km->prev, Rz * 8);
    T.raw(km->avg, Rz * 8);
    T.raw(km->code, Rz * N * 4);
    T.raw(km->psum, Rz * km->P * k * d * 8);
    T.raw(km->pcnt, Rz * km->P * k * 4);
    T.raw(km->pdist, Rz * km->NWA * 8);
    if (int rc = psi_blob_realise(T, &km->blob, "psi_kmeans_create")) {
        delete km;
        return rc;
    }
    const long n = (long)N * d;
    hipLaunchKernelGGL(km_transpose_kernel, dim3(psi_cdiv(n, KB)), dim3(KB), 0, 0, obs, n, N, d, km->obsT);
    hipLaunchKernelGGL(km_init_kernel, dim3(1), dim3(64), 0, 0, *km);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        psi_set_error("psi_kmeans_create failed: %s", hipGetErrorString(e));
        psi_kmeans_destroy(km);
        return (int)e;
    }
    *out = km;
    return 0;
}

extern "C" void psi_kmeans_destroy(psi_kmeans *km)
{
    if (!km) return;
    (void)hipFree(km->blob);
    delete km;
}

extern "C" int psi_kmeans_iterate(psi_kmeans *km, int n_iter, void *stream)
{
    PSI_REQUIRE(km && n_iter >= 0, "bad arguments");
    hipStream_t st = (hipStream_t)stream;
    for (int it = 0; it < n_iter; it++) {
        int rc = km_launch_assign<true>(km->obsT, km->N, km->d, km->book, (size_t)km->k * km->d, km->k_eff, km->k, km->conv, km->R, km->code,
                                        nullptr, km->pdist, st);
        if (rc) return rc;
        hipLaunchKernelGGL(km_update_kernel, dim3(km->P, km->k, km->R), dim3(KB), 0, st, *km);
        PSI_CHECK_LAUNCH("km_update_kernel");
        hipLaunchKernelGGL(km_finalize_kernel, dim3(km->R), dim3(KB), 0, st, *km);
        PSI_CHECK_LAUNCH("km_finalize_kernel");
    }
    return 0;
}

extern "C" int psi_kmeans_read(psi_kmeans *km, float *book, int32_t *k_eff, double *avg_dist, int32_t *iters, int *h_converged, void *stream)
{
    PSI_REQUIRE(km != nullptr, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t R = km->R;
    if (book) PSI_CHECK_HIP(hipMemcpyAsync(book, km->book, R * km->k * km->d * 4, hipMemcpyDeviceToDevice, st));
    if (k_eff) PSI_CHECK_HIP(hipMemcpyAsync(k_eff, km->k_eff, R * 4, hipMemcpyDeviceToDevice, st));
    if (avg_dist) PSI_CHECK_HIP(hipMemcpyAsync(avg_dist, km->avg, R * 8, hipMemcpyDeviceToDevice, st));
    if (iters) PSI_CHECK_HIP(hipMemcpyAsync(iters, km->iters, R * 4, hipMemcpyDeviceToDevice, st));
    if (h_converged) {
        std::vector<int> h(R);
        PSI_CHECK_HIP(hipMemcpyAsync(h.data(), km->conv, R * 4, hipMemcpyDeviceToHost, st));
        PSI_CHECK_HIP(hipStreamSynchronize(st));
        int n = 0;
        for (size_t r = 0; r < R; r++) n += h[r] != 0;
        *h_converged = n;
    }
    return 0;
}

extern "C" int psi_vq(const float *obs, int N, int d, const float *book, int k, int32_t *code, float *dist, void *stream)
{
    PSI_REQUIRE(obs && book && code, "null pointer");
    PSI_REQUIRE(N >= 1 && d >= 1 && d <= 128 && k >= 1 && k <= 64 && (long)N * d < (1L << 31), "d <= 128, k <= 64");
    return km_launch_assign<false>(obs, N, d, book, 0, nullptr, k, nullptr, 1, code, dist, nullptr, (hipStream_t)stream);
}
