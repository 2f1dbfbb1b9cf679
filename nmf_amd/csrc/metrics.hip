// Evaluation metrics of renderer.py:195-560 (evaluate): SSIM (utils.py:90-136, rgb_ssim) and the per-view normal error
// (renderer.py:357-390).  Neither is on the training path; both run once per test view.
//
// nmf_ssim: one launch for every view and channel.  A workgroup owns an output tile of SSIM_TH x SSIM_TW pixels of one view,
// stages the tile plus its 10-pixel halo of both images (all three channels, fp32) in LDS once, then per channel filters
// vertically into fp64 moments (LDS) and horizontally into the per-pixel formula.  The moments and the formula are fp64:
// in fp32 E[x^2] - mu^2 cancels against c2 = 9e-4 and the clamp at 0 turns the rounding into a bias.  x^2, y^2 and xy of
// fp32 inputs are exact in fp64.  Each workgroup writes the fp64 sum of its tile's map; k_view_reduce adds a view's
// partials in a fixed order (no atomics), so a view's value does not depend on the run or on the other views of the call.
//
// nmf_normal_err: fp32 per pixel, in the torch expression's operation order (this file is built with -ffp-contract=off);
// sums in fp64, reduced the same way.
#include "common.hpp"
#include <math.h>

namespace {

constexpr int SSIM_K = 11;                    // filter_size (the only one compiled)
constexpr int SSIM_TH = 16, SSIM_TW = 32;     // output tile
constexpr int SSIM_IH = SSIM_TH + SSIM_K - 1, SSIM_IW = SSIM_TW + SSIM_K - 1;
constexpr int SSIM_C = 3;
constexpr int SSIM_THREADS = 256;
// LDS: inputs 2 x 3 x 26 x 42 fp32 = 26208 B, vertical moments 5 x 16 x 42 fp64 = 26880 B -> 53088 B (two workgroups per CU)

struct SsimArgs {
    double taps[SSIM_K];
    double c1, c2;
};

__global__ __launch_bounds__(SSIM_THREADS) void k_ssim_tiles(const float* __restrict__ a, const float* __restrict__ b,
                                                              int32_t H, int32_t W, int32_t tiles_x, int32_t tiles_per_img,
                                                              SsimArgs args, double* __restrict__ partials,
                                                              float* __restrict__ map_out) {
    __shared__ float sA[SSIM_C][SSIM_IH][SSIM_IW];
    __shared__ float sB[SSIM_C][SSIM_IH][SSIM_IW];
    __shared__ double sV[5][SSIM_TH][SSIM_IW];
    __shared__ double sRed[SSIM_THREADS / NMF_WAVE];

    const int64_t blk = blockIdx.x;
    const int64_t img = blk / tiles_per_img;
    const int tile = (int)(blk - img * tiles_per_img);
    const int y0 = (tile / tiles_x) * SSIM_TH, x0 = (tile % tiles_x) * SSIM_TW;
    const int Ho = H - (SSIM_K - 1), Wo = W - (SSIM_K - 1);
    const int tid = threadIdx.x;
    const size_t img_off = (size_t)img * H * W * SSIM_C;

    // stage the tile + halo: a row of the tile is SSIM_IW * 3 consecutive floats in memory (coalesced), zero outside the image
    for (int i = tid; i < SSIM_IH * SSIM_IW * SSIM_C; i += SSIM_THREADS) {
        const int r = i / (SSIM_IW * SSIM_C), rem = i - r * (SSIM_IW * SSIM_C);
        const int c = rem / SSIM_C, ch = rem - c * SSIM_C;
        const int y = y0 + r, x = x0 + c;
        float va = 0.f, vb = 0.f;
        if (y < H && x < W) {
            const size_t g = img_off + ((size_t)y * W + x) * SSIM_C + ch;
            va = a[g];
            vb = b[g];
        }
        sA[ch][r][c] = va;
        sB[ch][r][c] = vb;
    }
    __syncthreads();

    double acc = 0.0;
    for (int ch = 0; ch < SSIM_C; ++ch) {
        // vertical pass (scipy convolve2d with filt[:, None], utils.py:110-113): SSIM_TH x SSIM_IW items
        for (int i = tid; i < SSIM_TH * SSIM_IW; i += SSIM_THREADS) {
            const int r = i / SSIM_IW, c = i - r * SSIM_IW;
            double m0 = 0, m1 = 0, m00 = 0, m11 = 0, m01 = 0;
#pragma unroll
            for (int t = 0; t < SSIM_K; ++t) {
                const double w = args.taps[t];
                const double x = (double)sA[ch][r + t][c], y = (double)sB[ch][r + t][c];
                m0 += w * x;
                m1 += w * y;
                m00 += w * (x * x);
                m11 += w * (y * y);
                m01 += w * (x * y);
            }
            sV[0][r][c] = m0;
            sV[1][r][c] = m1;
            sV[2][r][c] = m00;
            sV[3][r][c] = m11;
            sV[4][r][c] = m01;
        }
        __syncthreads();
        // horizontal pass (filt[None, :]) and the per-pixel formula (utils.py:116-135)
        for (int i = tid; i < SSIM_TH * SSIM_TW; i += SSIM_THREADS) {
            const int r = i / SSIM_TW, c = i - r * SSIM_TW;
            const int oy = y0 + r, ox = x0 + c;
            if (oy >= Ho || ox >= Wo) continue;
            double mu0 = 0, mu1 = 0, e00 = 0, e11 = 0, e01 = 0;
#pragma unroll
            for (int t = 0; t < SSIM_K; ++t) {
                const double w = args.taps[t];
                mu0 += w * sV[0][r][c + t];
                mu1 += w * sV[1][r][c + t];
                e00 += w * sV[2][r][c + t];
                e11 += w * sV[3][r][c + t];
                e01 += w * sV[4][r][c + t];
            }
            const double mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
            const double s00 = fmax(0.0, e00 - mu00);
            const double s11 = fmax(0.0, e11 - mu11);
            double s01 = e01 - mu01;
            const double lim = fmin(sqrt(s00 * s11), fabs(s01));
            s01 = s01 > 0.0 ? lim : (s01 < 0.0 ? -lim : 0.0);           // np.sign(s01) * min(.., |s01|)
            const double numer = (2.0 * mu01 + args.c1) * (2.0 * s01 + args.c2);
            const double denom = (mu00 + mu11 + args.c1) * (s00 + s11 + args.c2);
            const double v = numer / denom;
            acc += v;
            if (map_out) map_out[(((size_t)img * Ho + oy) * Wo + ox) * SSIM_C + ch] = (float)v;
        }
        __syncthreads();                                                // sV is rewritten by the next channel
    }

    // fixed-order block sum: DPP wave scan (same lanes every run), then the waves in order
    const double ws = wave_incl_scan_dpp(acc);
    const double wsum = __shfl(ws, NMF_WAVE - 1, NMF_WAVE);
    if (lane_id() == 0) sRed[tid / NMF_WAVE] = wsum;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < SSIM_THREADS / NMF_WAVE; ++w) s += sRed[w];
        partials[blk] = s;
    }
}

// ---- normal error (renderer.py:369-389) -------------------------------------------------------------------------------
constexpr int NERR_THREADS = 256;
constexpr int NERR_PER_THREAD = 16;
constexpr int NERR_PER_BLOCK = NERR_THREADS * NERR_PER_THREAD;

// (n * 127 + 128).int(), then (q - 128) / 127 -- false for a non-finite quantised value (float -> int of NaN / inf is
// platform-defined in torch; the pixel's error becomes NaN, which renderer.py:387 maps to 0)
__device__ __forceinline__ bool quant3(const float* __restrict__ n, float (&o)[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float s = n[k] * 127.0f + 128.0f;
        ok = ok && (fabsf(s) < 2147483520.0f);
        const int q = ok ? (int)s : 128;                                 // truncation toward zero, as torch .int()
        o[k] = (float)(q - 128) / 127.0f;
    }
    return ok;
}
__device__ __forceinline__ void renorm3(float (&v)[3]) {
    const float ss = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];           // (v ** 2).sum(-1)
    const float d = sqrtf(ss + 1e-6f);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = v[k] / d;
}

__global__ __launch_bounds__(NERR_THREADS) void k_normal_err(const float* __restrict__ pred, const float* __restrict__ gt,
                                                              const float* __restrict__ accm, int64_t n_px, int32_t blocks_per_img,
                                                              double* __restrict__ partials, float* __restrict__ err_map) {
    __shared__ double sRed[2][NERR_THREADS / NMF_WAVE];
    const int64_t blk = blockIdx.x;
    const int64_t img = blk / blocks_per_img;
    const int64_t p0 = (blk - img * blocks_per_img) * (int64_t)NERR_PER_BLOCK;
    const int tid = threadIdx.x;
    double s_err = 0.0, s_acc = 0.0;
    for (int j = 0; j < NERR_PER_THREAD; ++j) {
        const int64_t p = p0 + (int64_t)j * NERR_THREADS + tid;
        if (p >= n_px) break;
        const int64_t g = img * n_px + p;
        float pn[3], gn[3];
        const bool ok_p = quant3(pred + 3 * g, pn);
        const bool ok_g = quant3(gt + 3 * g, gn);
        const bool ok = ok_p && ok_g;
        renorm3(gn);
        renorm3(pn);
        float dot = pn[0] * gn[0] + pn[1] * gn[1] + pn[2] * gn[2];
        dot = fminf(fmaxf(dot, 1e-8f), 1.0f);                           // clip(min=1e-8, max=1 - 1e-8): 1.0 in fp32
        float err = acosf(dot) * 180.0f / 3.14159265358979323846f;
        if (!ok || isnan(err)) err = 0.0f;
        const float a = accm[g];
        err = err * a;
        if (err_map) err_map[g] = err;
        s_err += (double)err;
        s_acc += (double)a;
    }
    double w0 = wave_incl_scan_dpp(s_err), w1 = wave_incl_scan_dpp(s_acc);
    w0 = __shfl(w0, NMF_WAVE - 1, NMF_WAVE);
    w1 = __shfl(w1, NMF_WAVE - 1, NMF_WAVE);
    if (lane_id() == 0) {
        sRed[0][tid / NMF_WAVE] = w0;
        sRed[1][tid / NMF_WAVE] = w1;
    }
    __syncthreads();
    if (tid == 0) {
        double a0 = 0.0, a1 = 0.0;
        for (int w = 0; w < NERR_THREADS / NMF_WAVE; ++w) {
            a0 += sRed[0][w];
            a1 += sRed[1][w];
        }
        partials[2 * blk] = a0;
        partials[2 * blk + 1] = a1;
    }
}

// one workgroup per view: its `per_img` partials (stride `width` doubles) summed in a fixed order.
// width 1: out = sum / denom (SSIM mean); width 2: out = sum0 / sum1 (normal error, NaN when sum1 == 0 as in the reference)
constexpr int RED_THREADS = 256;
__global__ __launch_bounds__(RED_THREADS) void k_view_reduce(const double* __restrict__ partials, int32_t per_img, int32_t width,
                                                              double denom, double* __restrict__ out) {
    __shared__ double sRed[2][RED_THREADS / NMF_WAVE];
    const int64_t img = blockIdx.x;
    const int tid = threadIdx.x;
    const double* p = partials + img * (int64_t)per_img * width;
    double s0 = 0.0, s1 = 0.0;
    for (int i = tid; i < per_img; i += RED_THREADS) {
        s0 += p[(int64_t)i * width];
        if (width == 2) s1 += p[(int64_t)i * width + 1];
    }
    double w0 = wave_incl_scan_dpp(s0), w1 = wave_incl_scan_dpp(s1);
    w0 = __shfl(w0, NMF_WAVE - 1, NMF_WAVE);
    w1 = __shfl(w1, NMF_WAVE - 1, NMF_WAVE);
    if (lane_id() == 0) {
        sRed[0][tid / NMF_WAVE] = w0;
        sRed[1][tid / NMF_WAVE] = w1;
    }
    __syncthreads();
    if (tid == 0) {
        double a0 = 0.0, a1 = 0.0;
        for (int w = 0; w < RED_THREADS / NMF_WAVE; ++w) {
            a0 += sRed[0][w];
            a1 += sRed[1][w];
        }
        out[img] = width == 2 ? a0 / a1 : a0 / denom;
    }
}

int64_t ssim_tiles(int64_t H, int64_t W, int64_t* tiles_x) {
    const int64_t tx = cdiv(W - (SSIM_K - 1), SSIM_TW), ty = cdiv(H - (SSIM_K - 1), SSIM_TH);
    if (tiles_x) *tiles_x = tx;
    return tx * ty;
}

constexpr int64_t MAX_BLOCKS = INT32_MAX / 1024;      // grid.x * 256 stays below 2^31

}  // namespace

extern "C" int64_t nmf_ssim_workspace_bytes(int64_t n_img, int32_t H, int32_t W, int32_t C) {
    if (n_img <= 0 || H < SSIM_K || W < SSIM_K || C != SSIM_C) return 0;
    return n_img * ssim_tiles(H, W, nullptr) * (int64_t)sizeof(double);
}

extern "C" int nmf_ssim(const float* a, const float* b, int64_t n_img, int32_t H, int32_t W, int32_t C, const double* taps11,
                        double c1, double c2, double* mean_out, float* map_out, void* workspace, int64_t workspace_bytes,
                        void* stream) {
    NMF_REQUIRE(n_img >= 0, NMF_EINVAL, "nmf_ssim: n_img < 0");
    NMF_REQUIRE(H >= SSIM_K && W >= SSIM_K, NMF_EINVAL, "nmf_ssim: H and W must be >= 11 (filter_size)");
    NMF_REQUIRE(C == SSIM_C, NMF_ERANGE, "nmf_ssim: C must be 3");
    NMF_REQUIRE(taps11, NMF_EINVAL, "nmf_ssim: taps11 is null");
    if (n_img == 0) return NMF_OK;
    NMF_REQUIRE(a && b && mean_out && workspace, NMF_EINVAL, "nmf_ssim: null pointer");
    int64_t tiles_x = 0;
    const int64_t per_img = ssim_tiles(H, W, &tiles_x);
    NMF_REQUIRE(n_img * per_img <= MAX_BLOCKS, NMF_ERANGE, "nmf_ssim: too many tiles in one call");
    NMF_REQUIRE(workspace_bytes >= nmf_ssim_workspace_bytes(n_img, H, W, C), NMF_EINVAL, "nmf_ssim: workspace too small");
    SsimArgs args;
    for (int t = 0; t < SSIM_K; ++t) args.taps[t] = taps11[t];           // host array, read at call time
    args.c1 = c1;
    args.c2 = c2;
    double* partials = static_cast<double*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    NMF_LAUNCH(k_ssim_tiles, dim3((uint32_t)(n_img * per_img)), dim3(SSIM_THREADS), 0, s, a, b, H, W, (int32_t)tiles_x,
               (int32_t)per_img, args, partials, map_out);
    NMF_CHECK_LAUNCH("nmf_ssim: k_ssim_tiles");
    const double count = (double)(H - (SSIM_K - 1)) * (double)(W - (SSIM_K - 1)) * SSIM_C;
    NMF_LAUNCH(k_view_reduce, dim3((uint32_t)n_img), dim3(RED_THREADS), 0, s, (const double*)partials, (int32_t)per_img, 1,
               count, mean_out);
    NMF_CHECK_LAUNCH("nmf_ssim: k_view_reduce");
    return NMF_OK;
}

extern "C" int64_t nmf_normal_err_workspace_bytes(int64_t n_img, int64_t n_px) {
    if (n_img <= 0 || n_px <= 0) return 0;
    return n_img * cdiv(n_px, NERR_PER_BLOCK) * 2 * (int64_t)sizeof(double);
}

extern "C" int nmf_normal_err(const float* pred, const float* gt, const float* acc, int64_t n_img, int64_t n_px,
                              double* mean_out, float* err_map, void* workspace, int64_t workspace_bytes, void* stream) {
    NMF_REQUIRE(n_img >= 0, NMF_EINVAL, "nmf_normal_err: n_img < 0");
    if (n_img == 0) return NMF_OK;
    NMF_REQUIRE(n_px > 0, NMF_EINVAL, "nmf_normal_err: n_px must be > 0");
    NMF_REQUIRE(pred && gt && acc && mean_out && workspace, NMF_EINVAL, "nmf_normal_err: null pointer");
    const int64_t per_img = cdiv(n_px, NERR_PER_BLOCK);
    NMF_REQUIRE(n_img * per_img <= MAX_BLOCKS, NMF_ERANGE, "nmf_normal_err: too many pixels in one call");
    NMF_REQUIRE(workspace_bytes >= nmf_normal_err_workspace_bytes(n_img, n_px), NMF_EINVAL,
                "nmf_normal_err: workspace too small");
    double* partials = static_cast<double*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    NMF_LAUNCH(k_normal_err, dim3((uint32_t)(n_img * per_img)), dim3(NERR_THREADS), 0, s, pred, gt, acc, n_px,
               (int32_t)per_img, partials, err_map);
    NMF_CHECK_LAUNCH("nmf_normal_err: k_normal_err");
    NMF_LAUNCH(k_view_reduce, dim3((uint32_t)n_img), dim3(RED_THREADS), 0, s, (const double*)partials, (int32_t)per_img, 2,
               1.0, mean_out);
    NMF_CHECK_LAUNCH("nmf_normal_err: k_view_reduce");
    return NMF_OK;
}
