// Denoised frames (nmf_amd/multisample.py:FrameAccumulator.denoise; include/nmf_hip.h, "Denoised frames"): a
// spatial, edge-avoiding a-trous wavelet filter over the finished accumulator state of accum.hip -- the mean radiance, coverage and
// displayed colour of a multi-sample frame, steered by the per-pixel variance of the mean and stopped by the mean depth, normal and
// coverage.  The reference renders one sample per pixel and has none of this.
//
// Three kernels, one lane per pixel, plain loads and stores, no atomics, no LDS: two runs give the same bytes.  The planes of a
// 400 x 400 frame (state 9.6 MB, workspace 12.2 MB) stay in the Infinity Cache, and a wave's loads of one tap are 64 consecutive
// floats of a plane, so nothing is staged (DESIGN.md 10.12 has the measurement).  Every tap index is checked against the frame
// before anything is read through it.
//
// All three are restated in numpy fp32 by tests/test_denoise_cpu.py (denoise_np) and compared bit for bit: contraction is off, the
// only operations are + - * / fmaxf fabsf (one rounding each; '/' and sqrtf are hipcc's correctly rounded fp32 forms, as in
// accum.hip), and the displayed colour is accum.hip's own device function (accum_planes.hpp).
#include "accum_planes.hpp"

#pragma clang fp contract(off)

namespace {

using namespace accum;

constexpr int DN_BLOCK = 256;

// planes of the workspace, P 4-byte words each (NMF_DENOISE_PLANES of them): the pixels that pass through, the depth gradient, and
// two sets of the planes a level rewrites
enum { WS_FIXED = 0, WS_GX = 1, WS_GY = 2, WS_SET = 3 };
enum { V_LIN = 0, V_ACC = 3, V_MAP = 4, V_VAR = 7, V_END = 8 };      // planes of one set
static_assert(WS_SET + 2 * V_END == NMF_DENOISE_PLANES, "workspace planes");

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// se^2 of a pixel: max_c M2_c / (n (n - 1)), 0 below two samples (fmaxf drops a NaN quotient)
__device__ __forceinline__ float var_of_mean(const float* __restrict__ state, int64_t P, int64_t p) {
    const int32_t count = reinterpret_cast<const int32_t*>(state)[p];
    if (count < 2) return 0.f;
    const float cc = (float)count * (float)(count - 1);
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) v = fmaxf(v, state[(int64_t)(PL_M2 + k) * P + p] / cc);
    return v;
}

// ---- prepare -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DN_BLOCK) k_denoise_prepare(const float* __restrict__ state, float* __restrict__ ws, int H, int W) {
    const int64_t P = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int y = (int)((uint32_t)p / (uint32_t)W), x = (int)((uint32_t)p - (uint32_t)y * (uint32_t)W);      // P < 2^31
    const int xs[3] = {clampi(x - 1, W - 1), x, clampi(x + 1, W - 1)};
    const int ys[3] = {clampi(y - 1, H - 1), y, clampi(y + 1, H - 1)};
    // the 3 x 3 binomial blur of the variance, rows first: ((a + 2 b) + c) per row, the same over the rows, / 16
    float r[3];
    float v_own = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int64_t row = (int64_t)ys[j] * W;
        const float a = var_of_mean(state, P, row + xs[0]), b = var_of_mean(state, P, row + xs[1]), c = var_of_mean(state, P, row + xs[2]);
        if (j == 1) v_own = b;
        r[j] = (a + 2.f * b) + c;
    }
    const float vg = ((r[0] + 2.f * r[1]) + r[2]) * 0.0625f;
    const float* Z = state + (int64_t)PL_DEPTH * P;
    const float gx = (Z[(int64_t)y * W + xs[2]] - Z[(int64_t)y * W + xs[0]]) * 0.5f;
    const float gy = (Z[(int64_t)ys[2] * W + x] - Z[(int64_t)ys[0] * W + x]) * 0.5f;
    reinterpret_cast<int32_t*>(ws)[(int64_t)WS_FIXED * P + p] = v_own == 0.f ? 1 : 0;
    ws[(int64_t)WS_GX * P + p] = gx;
    ws[(int64_t)WS_GY * P + p] = gy;
    float* set = ws + (int64_t)WS_SET * P;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        set[(int64_t)(V_LIN + k) * P + p] = state[(int64_t)(PL_LIN + k) * P + p];
        set[(int64_t)(V_MAP + k) * P + p] = state[(int64_t)(PL_MAP + k) * P + p];
    }
    set[(int64_t)V_ACC * P + p] = state[(int64_t)PL_ACC * P + p];
    set[(int64_t)V_VAR * P + p] = vg;
}

// ---- one level ---------------------------------------------------------------------------------------------------------------------
struct LevelArgs {
    const float* state;      // the guides that are never filtered: mean normal and depth
    float* ws;
    int H, W;
    int step, src;           // the set that is read (0 / 1); the other one is written
    float kc2, kn2, kz, eps_z, ka2;
};

__global__ void __launch_bounds__(DN_BLOCK) k_denoise_level(LevelArgs A) {
    const int64_t P = (int64_t)A.H * A.W;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const float* __restrict__ in = A.ws + (int64_t)(WS_SET + A.src * V_END) * P;
    float* __restrict__ out = A.ws + (int64_t)(WS_SET + (1 - A.src) * V_END) * P;
    if (reinterpret_cast<const int32_t*>(A.ws)[(int64_t)WS_FIXED * P + p]) {      // passes through every level bit for bit
#pragma unroll
        for (int k = 0; k < V_END; ++k) out[(int64_t)k * P + p] = in[(int64_t)k * P + p];
        return;
    }
    const int y = (int)((uint32_t)p / (uint32_t)A.W), x = (int)((uint32_t)p - (uint32_t)y * (uint32_t)A.W);
    const float* __restrict__ N = A.state + (int64_t)PL_NORMAL * P;
    const float* __restrict__ Z = A.state + (int64_t)PL_DEPTH * P;
    const float cp0 = in[(int64_t)(V_MAP + 0) * P + p], cp1 = in[(int64_t)(V_MAP + 1) * P + p], cp2 = in[(int64_t)(V_MAP + 2) * P + p];
    const float np0 = N[p], np1 = N[P + p], np2 = N[2 * P + p];
    const float zp = Z[p], ap = in[(int64_t)V_ACC * P + p], vp = in[(int64_t)V_VAR * P + p];
    const float gx = A.ws[(int64_t)WS_GX * P + p], gy = A.ws[(int64_t)WS_GY * P + p];
    const float b[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.f, sv = 0.f, sl[3] = {0.f, 0.f, 0.f}, sa = 0.f, sc[3] = {0.f, 0.f, 0.f};
    int others = 0;                                                            // taps beside the centre that contributed
#pragma unroll
    for (int i = -2; i <= 2; ++i) {
        const int64_t qy = (int64_t)y + (int64_t)A.step * i;
        if (qy < 0 || qy >= A.H) continue;
#pragma unroll
        for (int j = -2; j <= 2; ++j) {
            const int64_t qx = (int64_t)x + (int64_t)A.step * j;
            if (qx < 0 || qx >= A.W) continue;
            const int64_t q = qy * A.W + qx;                                   // inside [0, P): both coordinates were checked
            float w = b[i + 2] * b[j + 2];                                      // (exact: 36 / 256 at the most)
            if (i != 0 || j != 0) {
                const float c0 = cp0 - in[(int64_t)(V_MAP + 0) * P + q], c1 = cp1 - in[(int64_t)(V_MAP + 1) * P + q],
                            c2 = cp2 - in[(int64_t)(V_MAP + 2) * P + q];
                float d = ((c0 * c0 + c1 * c1) + c2 * c2) / (A.kc2 * (vp + in[(int64_t)V_VAR * P + q]) + 1e-10f);
                const float n0 = np0 - N[q], n1 = np1 - N[P + q], n2 = np2 - N[2 * P + q];
                d = d + ((n0 * n0 + n1 * n1) + n2 * n2) / A.kn2;
                const float dz = zp - Z[q];
                const float e = A.kz * fabsf(gx * (float)(A.step * j) + gy * (float)(A.step * i)) + A.eps_z;
                d = d + (dz * dz) / (e * e);
                const float da = ap - in[(int64_t)V_ACC * P + q];
                d = d + (da * da) / A.ka2;
                const float t = fmaxf(0.f, 1.f - d);                            // (0 for a NaN)
                if (!(t > 0.f)) continue;                                       // compact support: the tap adds exactly nothing
                w = (w * t) * t;
                ++others;
            }
            sw = sw + w;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                sl[k] = sl[k] + w * in[(int64_t)(V_LIN + k) * P + q];
                sc[k] = sc[k] + w * in[(int64_t)(V_MAP + k) * P + q];
            }
            sa = sa + w * in[(int64_t)V_ACC * P + q];
            sv = sv + (w * w) * in[(int64_t)V_VAR * P + q];
        }
    }
    if (others == 0) {      // the centre alone: (h x) / h need not return x, so the pixel is copied like a fixed one
#pragma unroll
        for (int k = 0; k < V_END; ++k) out[(int64_t)k * P + p] = in[(int64_t)k * P + p];
        return;
    }
    // sw holds the centre's 36 / 256 at least
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out[(int64_t)(V_LIN + k) * P + p] = sl[k] / sw;
        out[(int64_t)(V_MAP + k) * P + p] = sc[k] / sw;
    }
    out[(int64_t)V_ACC * P + p] = sa / sw;
    out[(int64_t)V_VAR * P + p] = sv / (sw * sw);
}

// ---- finish ------------------------------------------------------------------------------------------------------------------------
struct FinishArgs {
    const float* ws;
    int64_t P;
    int src;
    float bg[3];
    int tonemap, noclip;
    float *rgb_map, *rgb_lin, *acc, *se;
};

__global__ void __launch_bounds__(DN_BLOCK) k_denoise_finish(FinishArgs A) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= A.P) return;
    const float* __restrict__ in = A.ws + (int64_t)(WS_SET + A.src * V_END) * A.P;
    const float a = in[(int64_t)V_ACC * A.P + p];
    const float t = 1.f - a;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = in[(int64_t)(V_LIN + k) * A.P + p];
        if (A.rgb_map) A.rgb_map[p * 3 + k] = displayed(v, t, A.bg[k], A.tonemap, A.noclip);
        if (A.rgb_lin) A.rgb_lin[p * 3 + k] = v;
    }
    if (A.acc) A.acc[p] = a;
    if (A.se) A.se[p] = sqrtf(in[(int64_t)V_VAR * A.P + p]);
}

inline bool positive_f(float v) { return v > 0.f && finite_f(v); }      // (false for a NaN)

// the checks of every entry point; `what` carries the function's name
int check_buffers(const void* state, const void* ws, bool need_state, const char* null_msg, const char* align_msg) {
    NMF_REQUIRE((state || !need_state) && ws, NMF_EINVAL, null_msg);
    NMF_REQUIRE(((uintptr_t)state & 3) == 0 && ((uintptr_t)ws & 3) == 0, NMF_EINVAL, align_msg);
    return NMF_OK;
}

}  // namespace

extern "C" int64_t nmf_denoise_workspace_bytes(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W > 2147483647LL) return 0;
    return 4 * (int64_t)NMF_DENOISE_PLANES * H * W;
}

extern "C" int nmf_denoise_prepare(const void* state, void* workspace, int32_t H, int32_t W, void* stream) {
    if (int rc = check_frame(H, W, "nmf_denoise_prepare: H or W below 1", "nmf_denoise_prepare: more than 2^31 - 1 pixels")) return rc;
    if (int rc = check_buffers(state, workspace, true, "nmf_denoise_prepare: null pointer",
                               "nmf_denoise_prepare: state and workspace must be 4-byte aligned")) return rc;
    const int64_t P = (int64_t)H * W;
    NMF_LAUNCH(k_denoise_prepare, dim3((unsigned)cdiv(P, DN_BLOCK)), dim3(DN_BLOCK), 0, (hipStream_t)stream,
               static_cast<const float*>(state), static_cast<float*>(workspace), (int)H, (int)W);
    NMF_CHECK_LAUNCH("nmf_denoise_prepare");
    return NMF_OK;
}

extern "C" int nmf_denoise_level(const void* state, void* workspace, int32_t H, int32_t W, int32_t step, int32_t src, float k_c,
                                 float k_n, float k_z, float eps_z, float k_a, void* stream) {
    if (int rc = check_frame(H, W, "nmf_denoise_level: H or W below 1", "nmf_denoise_level: more than 2^31 - 1 pixels")) return rc;
    NMF_REQUIRE(step >= 1 && step <= (1 << NMF_DENOISE_MAX_LEVELS), NMF_EINVAL, "nmf_denoise_level: step outside [1, 256]");
    NMF_REQUIRE(src == 0 || src == 1, NMF_EINVAL, "nmf_denoise_level: src is 0 or 1");
    NMF_REQUIRE(positive_f(k_c) && positive_f(k_n) && positive_f(k_z) && positive_f(eps_z) && positive_f(k_a), NMF_EINVAL,
                "nmf_denoise_level: k_c, k_n, k_z, eps_z and k_a must be finite and positive");
    if (int rc = check_buffers(state, workspace, true, "nmf_denoise_level: null pointer",
                               "nmf_denoise_level: state and workspace must be 4-byte aligned")) return rc;
    LevelArgs A;
    A.state = static_cast<const float*>(state); A.ws = static_cast<float*>(workspace);
    A.H = H; A.W = W; A.step = step; A.src = src;
    A.kc2 = k_c * k_c; A.kn2 = k_n * k_n; A.kz = k_z; A.eps_z = eps_z; A.ka2 = k_a * k_a;      // fp32 products, as the header states
    NMF_LAUNCH(k_denoise_level, dim3((unsigned)cdiv((int64_t)H * W, DN_BLOCK)), dim3(DN_BLOCK), 0, (hipStream_t)stream, A);
    NMF_CHECK_LAUNCH("nmf_denoise_level");
    return NMF_OK;
}

extern "C" int nmf_denoise_finish(const void* workspace, int32_t H, int32_t W, int32_t src, float bg_r, float bg_g, float bg_b,
                                  int32_t tonemap, int32_t noclip, float* rgb_map, float* rgb_lin, float* acc, float* se, void* stream) {
    if (int rc = check_frame(H, W, "nmf_denoise_finish: H or W below 1", "nmf_denoise_finish: more than 2^31 - 1 pixels")) return rc;
    NMF_REQUIRE(src == 0 || src == 1, NMF_EINVAL, "nmf_denoise_finish: src is 0 or 1");
    NMF_REQUIRE(finite_f(bg_r) && finite_f(bg_g) && finite_f(bg_b), NMF_EINVAL, "nmf_denoise_finish: bg must be finite");
    if (int rc = check_buffers(nullptr, workspace, false, "nmf_denoise_finish: null workspace",
                               "nmf_denoise_finish: the workspace must be 4-byte aligned")) return rc;
    NMF_REQUIRE(rgb_map || rgb_lin || acc || se, NMF_EINVAL, "nmf_denoise_finish: no output (all four are null)");
    FinishArgs A;
    A.ws = static_cast<const float*>(workspace); A.P = (int64_t)H * W; A.src = src;
    A.bg[0] = bg_r; A.bg[1] = bg_g; A.bg[2] = bg_b; A.tonemap = tonemap; A.noclip = noclip;
    A.rgb_map = rgb_map; A.rgb_lin = rgb_lin; A.acc = acc; A.se = se;
    NMF_LAUNCH(k_denoise_finish, dim3((unsigned)cdiv(A.P, DN_BLOCK)), dim3(DN_BLOCK), 0, (hipStream_t)stream, A);
    NMF_CHECK_LAUNCH("nmf_denoise_finish");
    return NMF_OK;
}

extern "C" int nmf_denoise(const void* state, void* workspace, int32_t H, int32_t W, int32_t levels, float k_c, float k_n, float k_z,
                           float eps_z, float k_a, float bg_r, float bg_g, float bg_b, int32_t tonemap, int32_t noclip, float* rgb_map,
                           float* rgb_lin, float* acc, float* se, void* stream) {
    // every refusal before the first launch
    if (int rc = check_frame(H, W, "nmf_denoise: H or W below 1", "nmf_denoise: more than 2^31 - 1 pixels")) return rc;
    NMF_REQUIRE(levels >= 0 && levels <= NMF_DENOISE_MAX_LEVELS, NMF_EINVAL, "nmf_denoise: levels outside [0, 8]");
    NMF_REQUIRE(positive_f(k_c) && positive_f(k_n) && positive_f(k_z) && positive_f(eps_z) && positive_f(k_a), NMF_EINVAL,
                "nmf_denoise: k_c, k_n, k_z, eps_z and k_a must be finite and positive");
    NMF_REQUIRE(finite_f(bg_r) && finite_f(bg_g) && finite_f(bg_b), NMF_EINVAL, "nmf_denoise: bg must be finite");
    if (int rc = check_buffers(state, workspace, true, "nmf_denoise: null pointer",
                               "nmf_denoise: state and workspace must be 4-byte aligned")) return rc;
    NMF_REQUIRE(rgb_map || rgb_lin || acc || se, NMF_EINVAL, "nmf_denoise: no output (all four are null)");
    if (int rc = nmf_denoise_prepare(state, workspace, H, W, stream)) return rc;
    for (int32_t l = 0; l < levels; ++l) {
        if (int rc = nmf_denoise_level(state, workspace, H, W, 1 << l, l & 1, k_c, k_n, k_z, eps_z, k_a, stream)) return rc;
    }
    return nmf_denoise_finish(workspace, H, W, levels & 1, bg_r, bg_g, bg_b, tonemap, noclip, rgb_map, rgb_lin, acc, se, stream);
}
