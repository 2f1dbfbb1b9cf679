// Relighting evaluation (nmf_amd/relight_eval.py): the pixel arithmetic of the reference's scripts/relighting_calc.ipynb
// and of the HDR frame its renderer.py:425-429 stores.
//
//   nmf_relight_frame   rgb_lin, acc -> srgb_inverse(srgb_noclip(rgb_lin) + (1 - acc)), the linear frame on a white background
//   nmf_relight_ratio   per image and channel the sum of gt_c / max(pred_c, 1e-7) over the masked pixels, and their count
//   nmf_relight_adjust  pred * multi blended onto white with the ground-truth alpha, both sides tonemapped and clipped, their squared
//                       error per image
//
// Bandwidth-bound with a powf per value.  One thread per pixel: a pixel's three floats are one 12-byte access, consecutive lanes read
// consecutive pixels, the RGBA ground truth is one float4.  Sums are double: a thread adds its pixels in pixel order, a wave adds its
// lanes with shuffles, thread 0 adds the workgroup's waves in wave order and stores ONE partial per workgroup; a second kernel adds an
// image's partials in the same fixed way.  No atomics, no ticket: the same bytes on every run.  Contraction is off so that the numpy
// restatement of tests/relight_eval_ref.py follows the expression order below and differs by powf only.
#include <cmath>

#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int RL_THREADS = 256;
constexpr int RL_PER_THREAD = 8;
constexpr int RL_PER_BLOCK = RL_THREADS * RL_PER_THREAD;
constexpr int RL_WAVES = RL_THREADS / NMF_WAVE;
constexpr int64_t RL_MAX_BLOCKS = INT32_MAX / 1024;

constexpr float SRGB_FWD_LIMIT = 0.0031308f;
constexpr float SRGB_INV_LIMIT = 0.04045f;

// modules/tonemap.py:38-47 without the clip
__device__ __forceinline__ float srgb_noclip(float x) {
    return x > SRGB_FWD_LIMIT ? 1.055f * powf(fmaxf(x, SRGB_FWD_LIMIT), 1.0f / 2.4f) - 0.055f : 12.92f * x;
}

__device__ __forceinline__ float srgb_clip(float x) { return fminf(fmaxf(srgb_noclip(x), 0.f), 1.f); }

// modules/tonemap.py:49-55
__device__ __forceinline__ float srgb_inverse(float y) {
    return y > SRGB_INV_LIMIT ? powf((y + 0.055f) / 1.055f, 2.4f) : y / 12.92f;
}

__global__ void __launch_bounds__(RL_THREADS) k_relight_frame(const float* __restrict__ rgb_lin, const float* __restrict__ acc,
                                                             int64_t n, float* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * RL_THREADS + threadIdx.x;
    if (p >= n) return;
    const float t = 1.f - acc[p];
    const float x0 = rgb_lin[3 * p], x1 = rgb_lin[3 * p + 1], x2 = rgb_lin[3 * p + 2];
    out[3 * p] = srgb_inverse(srgb_noclip(x0) + t);
    out[3 * p + 1] = srgb_inverse(srgb_noclip(x1) + t);
    out[3 * p + 2] = srgb_inverse(srgb_noclip(x2) + t);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = NMF_WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, NMF_WAVE);
    return v;
}

// K doubles per thread -> K doubles at dst[0..K), written by thread 0: lanes by shuffle, waves in wave order
template <int K>
__device__ __forceinline__ void block_sum_store(const double (&s)[K], double* __restrict__ dst) {
    __shared__ double sRed[K][RL_WAVES];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double w = wave_sum(s[k]);
        if ((tid & (NMF_WAVE - 1)) == 0) sRed[k][tid / NMF_WAVE] = w;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double a = 0.0;
            for (int w = 0; w < RL_WAVES; ++w) a += sRed[k][w];
            dst[k] = a;
        }
    }
}

// partials [n_img * per_img][4]: three ratio sums and the count (a whole number below 2^53, exact in a double)
__global__ void __launch_bounds__(RL_THREADS) k_relight_ratio(const float* __restrict__ pred, const float4* __restrict__ gt,
                                                             int64_t n_px, int32_t per_img, double* __restrict__ partials) {
    const int64_t blk = blockIdx.x;
    const int64_t img = blk / per_img;
    const int64_t p0 = (blk - img * per_img) * (int64_t)RL_PER_BLOCK;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < RL_PER_THREAD; ++j) {
        const int64_t p = p0 + (int64_t)j * RL_THREADS + threadIdx.x;
        if (p >= n_px) break;
        const int64_t g = img * n_px + p;
        const float4 t = gt[g];
        const float a0 = pred[3 * g], a1 = pred[3 * g + 1], a2 = pred[3 * g + 2];
        // notebook cell lines 233-234: gt alpha > 0.5 and min_c pred_c > 0.01, both strict (a NaN fails either)
        if (t.w > 0.5f && a0 > 0.01f && a1 > 0.01f && a2 > 0.01f) {
            s[0] += (double)(t.x / fmaxf(a0, 1e-7f));
            s[1] += (double)(t.y / fmaxf(a1, 1e-7f));
            s[2] += (double)(t.z / fmaxf(a2, 1e-7f));
            s[3] += 1.0;
        }
    }
    block_sum_store<4>(s, partials + 4 * blk);
}

__global__ void __launch_bounds__(RL_THREADS) k_relight_adjust(const float* __restrict__ pred, const float4* __restrict__ gt,
                                                              float m0, float m1, float m2, int64_t n_px, int32_t per_img,
                                                              float* __restrict__ tp, float* __restrict__ tg,
                                                              double* __restrict__ partials) {
    const int64_t blk = blockIdx.x;
    const int64_t img = blk / per_img;
    const int64_t p0 = (blk - img * per_img) * (int64_t)RL_PER_BLOCK;
    double s[1] = {0.0};
    for (int j = 0; j < RL_PER_THREAD; ++j) {
        const int64_t p = p0 + (int64_t)j * RL_THREADS + threadIdx.x;
        if (p >= n_px) break;
        const int64_t g = img * n_px + p;
        const float4 t = gt[g];
        const float a = t.w, w = 1.f - a;
        // notebook cell lines 244-246
        const float q0 = srgb_clip((pred[3 * g] * m0) * a + w);
        const float q1 = srgb_clip((pred[3 * g + 1] * m1) * a + w);
        const float q2 = srgb_clip((pred[3 * g + 2] * m2) * a + w);
        const float r0 = srgb_clip(t.x + w), r1 = srgb_clip(t.y + w), r2 = srgb_clip(t.z + w);
        tp[3 * g] = q0; tp[3 * g + 1] = q1; tp[3 * g + 2] = q2;
        tg[3 * g] = r0; tg[3 * g + 1] = r1; tg[3 * g + 2] = r2;
        const float d0 = q0 - r0, d1 = q1 - r1, d2 = q2 - r2;
        s[0] += (double)(d0 * d0);
        s[0] += (double)(d1 * d1);
        s[0] += (double)(d2 * d2);
    }
    block_sum_store<1>(s, partials + blk);
}

// one workgroup per image: its per_img partials of K doubles.  K == 4: three sums and the count; K == 1: the squared error
template <int K>
__global__ void __launch_bounds__(RL_THREADS) k_relight_reduce(const double* __restrict__ partials, int32_t per_img,
                                                              double* __restrict__ out, int64_t* __restrict__ count) {
    __shared__ double sOut[K];
    const int64_t img = blockIdx.x;
    const double* p = partials + img * (int64_t)per_img * K;
    double s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    for (int i = threadIdx.x; i < per_img; i += RL_THREADS) {
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += p[(int64_t)i * K + k];
    }
    block_sum_store<K>(s, sOut);
    if (threadIdx.x == 0) {
        if (K == 4) {
            out[3 * img] = sOut[0]; out[3 * img + 1] = sOut[1]; out[3 * img + 2] = sOut[2];
            count[img] = (int64_t)sOut[3];
        } else {
            out[img] = sOut[0];
        }
    }
}

// n_img * H * W pixels and the workgroups of a reducing call, or a negative code
int relight_sizes(const char* who, int64_t n_img, int64_t H, int64_t W, int64_t* n_px, int64_t* per_img) {
    char msg[96];
    if (n_img < 1 || H < 1 || W < 1) {
        snprintf(msg, sizeof(msg), "%s: n_img, H and W must be at least 1", who);
        return nmf_fail(NMF_EINVAL, msg);
    }
    // (each factor below 2^31 first: the products cannot wrap)
    const bool fits = n_img <= INT32_MAX && H <= INT32_MAX && W <= INT32_MAX && H * W <= INT32_MAX &&
                      n_img * cdiv(H * W, RL_PER_BLOCK) <= RL_MAX_BLOCKS && cdiv(n_img * H * W, RL_THREADS) <= INT32_MAX;
    if (!fits) {
        snprintf(msg, sizeof(msg), "%s: too many pixels in one call", who);
        return nmf_fail(NMF_ERANGE, msg);
    }
    *n_px = H * W;
    *per_img = cdiv(H * W, RL_PER_BLOCK);
    return NMF_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int nmf_relight_frame(const float* rgb_lin, const float* acc, int64_t n_img, int64_t H, int64_t W, float* out,
                                 void* stream) {
    NMF_REQUIRE(rgb_lin && acc && out, NMF_EINVAL, "nmf_relight_frame: null pointer");
    int64_t n_px = 0, per_img = 0;
    if (int rc = relight_sizes("nmf_relight_frame", n_img, H, W, &n_px, &per_img)) return rc;
    const int64_t n = n_img * n_px;
    NMF_LAUNCH(k_relight_frame, dim3((uint32_t)cdiv(n, RL_THREADS)), dim3(RL_THREADS), 0, (hipStream_t)stream, rgb_lin, acc, n, out);
    NMF_CHECK_LAUNCH("nmf_relight_frame");
    return NMF_OK;
}

extern "C" int64_t nmf_relight_ratio_workspace_bytes(int64_t n_img, int64_t H, int64_t W) {
    int64_t n_px = 0, per_img = 0;
    if (relight_sizes("nmf_relight_ratio_workspace_bytes", n_img, H, W, &n_px, &per_img)) return 0;
    return n_img * per_img * 4 * (int64_t)sizeof(double);
}

extern "C" int nmf_relight_ratio(const float* pred, const float* gt, int64_t n_img, int64_t H, int64_t W, double* sum,
                                 int64_t* count, void* workspace, int64_t workspace_bytes, void* stream) {
    NMF_REQUIRE(pred && gt && sum && count && workspace, NMF_EINVAL, "nmf_relight_ratio: null pointer");
    int64_t n_px = 0, per_img = 0;
    if (int rc = relight_sizes("nmf_relight_ratio", n_img, H, W, &n_px, &per_img)) return rc;
    NMF_REQUIRE(aligned16(gt) && aligned16(workspace), NMF_EINVAL, "nmf_relight_ratio: gt and workspace must be 16-byte aligned");
    NMF_REQUIRE(workspace_bytes >= nmf_relight_ratio_workspace_bytes(n_img, H, W), NMF_EINVAL,
                "nmf_relight_ratio: workspace too small");
    double* partials = static_cast<double*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    NMF_LAUNCH(k_relight_ratio, dim3((uint32_t)(n_img * per_img)), dim3(RL_THREADS), 0, s, pred, reinterpret_cast<const float4*>(gt),
               n_px, (int32_t)per_img, partials);
    NMF_CHECK_LAUNCH("nmf_relight_ratio: k_relight_ratio");
    NMF_LAUNCH(k_relight_reduce<4>, dim3((uint32_t)n_img), dim3(RL_THREADS), 0, s, (const double*)partials, (int32_t)per_img, sum,
               count);
    NMF_CHECK_LAUNCH("nmf_relight_ratio: k_relight_reduce");
    return NMF_OK;
}

extern "C" int64_t nmf_relight_adjust_workspace_bytes(int64_t n_img, int64_t H, int64_t W) {
    int64_t n_px = 0, per_img = 0;
    if (relight_sizes("nmf_relight_adjust_workspace_bytes", n_img, H, W, &n_px, &per_img)) return 0;
    return n_img * per_img * (int64_t)sizeof(double);
}

extern "C" int nmf_relight_adjust(const float* pred, const float* gt, float multi_r, float multi_g, float multi_b, int64_t n_img,
                                  int64_t H, int64_t W, float* tp, float* tg, double* sqerr, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    NMF_REQUIRE(pred && gt && tp && tg && sqerr && workspace, NMF_EINVAL, "nmf_relight_adjust: null pointer");
    int64_t n_px = 0, per_img = 0;
    if (int rc = relight_sizes("nmf_relight_adjust", n_img, H, W, &n_px, &per_img)) return rc;
    NMF_REQUIRE(std::isfinite(multi_r) && std::isfinite(multi_g) && std::isfinite(multi_b), NMF_EINVAL,
                "nmf_relight_adjust: the multiplier is not finite");
    NMF_REQUIRE(aligned16(gt) && aligned16(workspace), NMF_EINVAL, "nmf_relight_adjust: gt and workspace must be 16-byte aligned");
    NMF_REQUIRE(workspace_bytes >= nmf_relight_adjust_workspace_bytes(n_img, H, W), NMF_EINVAL,
                "nmf_relight_adjust: workspace too small");
    double* partials = static_cast<double*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    NMF_LAUNCH(k_relight_adjust, dim3((uint32_t)(n_img * per_img)), dim3(RL_THREADS), 0, s, pred,
               reinterpret_cast<const float4*>(gt), multi_r, multi_g, multi_b, n_px, (int32_t)per_img, tp, tg, partials);
    NMF_CHECK_LAUNCH("nmf_relight_adjust: k_relight_adjust");
    NMF_LAUNCH(k_relight_reduce<1>, dim3((uint32_t)n_img), dim3(RL_THREADS), 0, s, (const double*)partials, (int32_t)per_img, sqerr,
               (int64_t*)nullptr);
    NMF_CHECK_LAUNCH("nmf_relight_adjust: k_relight_reduce");
    return NMF_OK;
}
