// Multi-sample frames (nmf_amd/multisample.py:render_frame; include/nmf_hip.h, "Multi-sample frames"): the rays of a
// pixel list at a sub-pixel offset, the per-pixel running statistics of the passes (Welford), the ascending list of the pixels that
// still need samples, and the finished maps.  The reference renders one sample per pixel and has none of this.
//
// One lane per pixel or list entry, plain vector loads and stores.  The list is a two-pass compaction (per-tile counts, a scan of
// the tile counts, a second pass that writes at the scanned offsets): nothing is appended in an order atomics decide, so the list is
// np.flatnonzero of the predicate on every run.  Every pixel id read from a list is checked against the frame before it indexes.
//
// All four are restated in numpy fp32 by the tests (tests/test_multisample_cpu.py) and compared bit for bit: contraction is off, '/'
// and sqrtf are hipcc's correctly rounded fp32 forms (as in camera.hip), and the one power of the tonemap is taken in double and
// rounded to fp32 once, which is the correctly rounded fp32 power wherever the double result is not within an ulp (of double) of
// a rounding boundary -- numpy's route is the same.
#include "accum_planes.hpp"

#pragma clang fp contract(off)

namespace {

using namespace accum;      // the planes of the state, finite_f, check_frame, srgb / displayed (shared with denoise.hip)

constexpr int ACC_BLOCK = 256;                 // lanes of a workgroup = pixels of a scan tile (NMF_ACCUM_TILE)
static_assert(ACC_BLOCK == NMF_ACCUM_TILE, "the tile of the list is one workgroup");

__device__ __forceinline__ float nan0(float v) { return v != v ? 0.f : v; }

// ---- rays of a pixel list ----------------------------------------------------------------------------------------------------------
struct RaysAtArgs {
    float r[9];
    float t[3];
    float fx, fy, cx, cy, jx, jy;
    uint32_t seed;
    int W;
    int64_t P, n;          // pixels of the frame; rows of `rays` (P when pix is null)
    const int32_t* pix;
    float* rays;           // [n][6]
};

__device__ __forceinline__ uint32_t mix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

__device__ __forceinline__ float wrap01(float j, uint32_t h) {
    float o = j + (float)(h >> 8) * (1.0f / 16777216.0f);
    if (o >= 1.f) o = o - 1.f;
    return o;
}

__global__ void __launch_bounds__(ACC_BLOCK) k_camera_rays_at(RaysAtArgs A) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    int64_t p = i;
    if (A.pix) {
        p = A.pix[i];
        if (p < 0 || p >= A.P) return;                                                   // the row keeps what it held
    }
    const uint32_t row = (uint32_t)p / (uint32_t)A.W, col = (uint32_t)p - row * (uint32_t)A.W;      // P < 2^31: 32-bit division
    float ox = A.jx, oy = A.jy;
    if (A.seed != 0u) {
        const uint32_t h0 = mix32((uint32_t)p * 0x9E3779B1u + A.seed * 0x85EBCA77u);
        const uint32_t h1 = mix32(h0 + 0x9E3779B9u);
        ox = wrap01(A.jx, h0);
        oy = wrap01(A.jy, h1);
    }
    const float x = (((float)col + ox) - A.cx) / A.fx;
    const float y = (((float)row + oy) - A.cy) / A.fy;
    const float n = sqrtf((x * x + y * y) + 1.f);
    const float dx = x / n, dy = y / n, dz = 1.f / n;
    const float w0 = (A.r[0] * dx + A.r[1] * dy) + A.r[2] * dz;
    const float w1 = (A.r[3] * dx + A.r[4] * dy) + A.r[5] * dz;
    const float w2 = (A.r[6] * dx + A.r[7] * dy) + A.r[8] * dz;
    float2* o = reinterpret_cast<float2*>(A.rays + i * 6);
    o[0] = make_float2(A.t[0], A.t[1]);
    o[1] = make_float2(A.t[2], w0);
    o[2] = make_float2(w1, w2);
}

// ---- Welford update ----------------------------------------------------------------------------------------------------------------
struct UpdateArgs {
    float* state;
    int64_t P, n;
    const int32_t* pix;
    const float *rgb_lin, *acc, *rgb_map, *depth, *normal;
};

__device__ __forceinline__ float* plane(float* state, int64_t P, int k) { return state + (int64_t)k * P; }

// mean += (x - mean) / c; returns the deviation from the OLD mean
__device__ __forceinline__ float fold(float* m, float x, float c) {
    const float old = *m, d = x - old;
    *m = old + d / c;
    return d;
}

__global__ void __launch_bounds__(ACC_BLOCK) k_accum_update(UpdateArgs A) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    int64_t p = i;
    if (A.pix) {
        p = A.pix[i];
        if (p < 0 || p >= A.P) return;
    }
    int32_t* cnt = reinterpret_cast<int32_t*>(A.state) + p;
    const int32_t c0 = *cnt;
    if (c0 < 0 || c0 == INT32_MAX) return;                                               // a count that cannot grow: the pixel is left alone
    const int32_t ci = c0 + 1;
    *cnt = ci;
    const float c = (float)ci;
#pragma unroll
    for (int k = 0; k < 3; ++k) fold(plane(A.state, A.P, PL_LIN + k) + p, nan0(A.rgb_lin[i * 3 + k]), c);
    fold(plane(A.state, A.P, PL_ACC) + p, nan0(A.acc[i]), c);
    if (A.depth) fold(plane(A.state, A.P, PL_DEPTH) + p, nan0(A.depth[i]), c);
    if (A.normal) {
#pragma unroll
        for (int k = 0; k < 3; ++k) fold(plane(A.state, A.P, PL_NORMAL + k) + p, nan0(A.normal[i * 3 + k]), c);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float* m = plane(A.state, A.P, PL_MAP + k) + p;
        const float x = nan0(A.rgb_map[i * 3 + k]);
        const float d = fold(m, x, c);
        float* m2 = plane(A.state, A.P, PL_M2 + k) + p;
        *m2 = *m2 + d * (x - *m);
    }
}

// ---- the standard error and the list ----------------------------------------------------------------------------------------------
// max_c sqrt(M2_c / (count (count - 1))), 0 below two samples
__device__ __forceinline__ float std_err(const float* state, int64_t P, int64_t p, int32_t count) {
    if (count < 2) return 0.f;
    const float cc = (float)count * (float)(count - 1);
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) se = fmaxf(se, sqrtf(state[(int64_t)(PL_M2 + k) * P + p] / cc));      // (fmaxf drops a NaN operand)
    return se;
}

__device__ __forceinline__ bool is_active(const float* state, int64_t P, int64_t p, int32_t min_spp, int32_t max_spp, float tol) {
    const int32_t count = reinterpret_cast<const int32_t*>(state)[p];
    if (count < min_spp) return true;
    return count < max_spp && std_err(state, P, p, count) > tol;
}

__device__ __forceinline__ int wave_incl_scan_i32(int v) {
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < NMF_WAVE; d <<= 1) {
        const int t = __shfl_up(v, d, NMF_WAVE);
        if (lane >= d) v += t;
    }
    return v;
}

// pass 1: the number of active pixels of every tile
__global__ void __launch_bounds__(ACC_BLOCK) k_active_count(const float* __restrict__ state, int64_t P, int32_t min_spp, int32_t max_spp,
                                                            float tol, int32_t* __restrict__ tiles) {
    __shared__ int wave_n[ACC_BLOCK / NMF_WAVE];
    const int64_t p = (int64_t)blockIdx.x * ACC_BLOCK + threadIdx.x;
    const bool on = p < P && is_active(state, P, p, min_spp, max_spp, tol);
    const uint64_t mask = __ballot(on);
    if (lane_id() == 0) wave_n[threadIdx.x / NMF_WAVE] = __popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < ACC_BLOCK / NMF_WAVE; ++w) s += wave_n[w];
        tiles[blockIdx.x] = s;
    }
}

// the scan: ONE workgroup walks the tile counts 256 at a time and leaves the EXCLUSIVE sums in their place, the total in n_out
__global__ void __launch_bounds__(ACC_BLOCK) k_active_scan(int32_t* __restrict__ tiles, int64_t n_tiles, int32_t* __restrict__ n_out) {
    __shared__ int wave_sum[ACC_BLOCK / NMF_WAVE];
    int carry = 0;
    for (int64_t base = 0; base < n_tiles; base += ACC_BLOCK) {
        const int64_t t = base + threadIdx.x;
        const int v = t < n_tiles ? tiles[t] : 0;
        const int incl = wave_incl_scan_i32(v);
        if (lane_id() == NMF_WAVE - 1) wave_sum[threadIdx.x / NMF_WAVE] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < ACC_BLOCK / NMF_WAVE; ++w) {
            if (w < (int)(threadIdx.x / NMF_WAVE)) before += wave_sum[w];
            total += wave_sum[w];
        }
        if (t < n_tiles) tiles[t] = carry + before + (incl - v);
        carry += total;
        __syncthreads();                                                                 // wave_sum is rewritten by the next round
    }
    if (threadIdx.x == 0) *n_out = carry;
}

// pass 2: the predicate again, the place inside the tile by ballot, the store at the tile's scanned offset
__global__ void __launch_bounds__(ACC_BLOCK) k_active_emit(const float* __restrict__ state, int64_t P, int32_t min_spp, int32_t max_spp,
                                                           float tol, const int32_t* __restrict__ tiles, int32_t* __restrict__ list) {
    __shared__ int wave_n[ACC_BLOCK / NMF_WAVE];
    const int64_t p = (int64_t)blockIdx.x * ACC_BLOCK + threadIdx.x;
    const bool on = p < P && is_active(state, P, p, min_spp, max_spp, tol);
    const uint64_t mask = __ballot(on);
    const int wave = threadIdx.x / NMF_WAVE;
    if (lane_id() == 0) wave_n[wave] = __popcll(mask);
    __syncthreads();
    if (!on) return;
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wave_n[w];
    const int64_t at = (int64_t)tiles[blockIdx.x] + before + __popcll(mask & ((1ull << lane_id()) - 1ull));
    if (at >= 0 && at < P) list[at] = (int32_t)p;                                         // (a list holds at most P entries)
}

// ---- the finished maps -------------------------------------------------------------------------------------------------------------
struct ResolveArgs {
    const float* state;
    int64_t P;
    float bg[3];
    int tonemap, noclip;
    float *rgb_map, *acc, *depth, *normal, *se, *count;
};

__global__ void __launch_bounds__(ACC_BLOCK) k_accum_resolve(ResolveArgs A) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= A.P) return;
    const int32_t count = reinterpret_cast<const int32_t*>(A.state)[p];
    const float a = A.state[(int64_t)PL_ACC * A.P + p];
    if (A.rgb_map) {
        const float t = 1.f - a;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = A.state[(int64_t)(PL_LIN + k) * A.P + p];
            A.rgb_map[p * 3 + k] = displayed(v, t, A.bg[k], A.tonemap, A.noclip);
        }
    }
    if (A.acc) A.acc[p] = a;
    if (A.depth) A.depth[p] = A.state[(int64_t)PL_DEPTH * A.P + p];
    if (A.normal) {
#pragma unroll
        for (int k = 0; k < 3; ++k) A.normal[p * 3 + k] = A.state[(int64_t)(PL_NORMAL + k) * A.P + p];
    }
    if (A.se) A.se[p] = std_err(A.state, A.P, p, count);
    if (A.count) A.count[p] = (float)count;
}

}  // namespace

extern "C" int64_t nmf_accum_state_bytes(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W > 2147483647LL) return 0;
    const int64_t P = (int64_t)H * W;
    return 4 * (NMF_ACCUM_PLANES * P + cdiv(P, NMF_ACCUM_TILE));
}

extern "C" int nmf_camera_rays_at(float r00, float r01, float r02, float r10, float r11, float r12, float r20, float r21, float r22,
                                  float tx, float ty, float tz, float fx, float fy, float cx, float cy, int32_t H, int32_t W, float jx,
                                  float jy, uint32_t seed, const int32_t* pix, int64_t n, float* rays, void* stream) {
    NMF_REQUIRE(H >= 1 && W >= 1, NMF_EINVAL, "nmf_camera_rays_at: H or W below 1");
    NMF_REQUIRE(finite_f(fx) && finite_f(fy) && fx != 0.f && fy != 0.f, NMF_EINVAL,
                "nmf_camera_rays_at: fx and fy must be finite and non-zero");
    const float pose[12] = {r00, r01, r02, r10, r11, r12, r20, r21, r22, tx, ty, tz};
    bool finite = finite_f(cx) && finite_f(cy);
    for (int k = 0; k < 12; ++k) finite = finite && finite_f(pose[k]);
    NMF_REQUIRE(finite, NMF_EINVAL, "nmf_camera_rays_at: the pose, cx and cy must be finite");
    NMF_REQUIRE(jx >= 0.f && jx <= 1.f && jy >= 0.f && jy <= 1.f, NMF_EINVAL, "nmf_camera_rays_at: the offset must lie in [0, 1]");
    NMF_REQUIRE(n >= 0, NMF_EINVAL, "nmf_camera_rays_at: n below 0");
    NMF_REQUIRE((int64_t)H * W <= 2147483647LL, NMF_ERANGE, "nmf_camera_rays_at: more than 2^31 - 1 pixels");
    NMF_REQUIRE(n <= 2147483647LL, NMF_ERANGE, "nmf_camera_rays_at: more than 2^31 - 1 list entries");
    RaysAtArgs A;
    A.P = (int64_t)H * W;
    A.n = pix ? n : A.P;
    if (A.n == 0) return NMF_OK;
    NMF_REQUIRE(rays, NMF_EINVAL, "nmf_camera_rays_at: null pointer");
    NMF_REQUIRE(((uintptr_t)rays & 7) == 0, NMF_EINVAL, "nmf_camera_rays_at: rays must be 8-byte aligned");
    for (int k = 0; k < 9; ++k) A.r[k] = pose[k];
    for (int k = 0; k < 3; ++k) A.t[k] = pose[9 + k];
    A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.jx = jx; A.jy = jy; A.seed = seed; A.W = W; A.pix = pix; A.rays = rays;
    NMF_LAUNCH(k_camera_rays_at, dim3((unsigned)cdiv(A.n, ACC_BLOCK)), dim3(ACC_BLOCK), 0, (hipStream_t)stream, A);
    NMF_CHECK_LAUNCH("nmf_camera_rays_at");
    return NMF_OK;
}

extern "C" int nmf_accum_update(void* state, int32_t H, int32_t W, const int32_t* pix, int64_t n, const float* rgb_lin, const float* acc,
                                const float* rgb_map, const float* depth, const float* normal, void* stream) {
    if (int rc = check_frame(H, W, "nmf_accum_update: H or W below 1", "nmf_accum_update: more than 2^31 - 1 pixels")) return rc;
    NMF_REQUIRE(n >= 0, NMF_EINVAL, "nmf_accum_update: n below 0");
    NMF_REQUIRE(n <= 2147483647LL, NMF_ERANGE, "nmf_accum_update: more than 2^31 - 1 list entries");
    UpdateArgs A;
    A.P = (int64_t)H * W;
    A.n = pix ? n : A.P;
    if (A.n == 0) return NMF_OK;
    NMF_REQUIRE(state && rgb_lin && acc && rgb_map, NMF_EINVAL, "nmf_accum_update: null pointer");
    NMF_REQUIRE(((uintptr_t)state & 3) == 0, NMF_EINVAL, "nmf_accum_update: state must be 4-byte aligned");
    A.state = static_cast<float*>(state); A.pix = pix;
    A.rgb_lin = rgb_lin; A.acc = acc; A.rgb_map = rgb_map; A.depth = depth; A.normal = normal;
    NMF_LAUNCH(k_accum_update, dim3((unsigned)cdiv(A.n, ACC_BLOCK)), dim3(ACC_BLOCK), 0, (hipStream_t)stream, A);
    NMF_CHECK_LAUNCH("nmf_accum_update");
    return NMF_OK;
}

extern "C" int nmf_accum_active(void* state, int32_t H, int32_t W, int32_t min_spp, int32_t max_spp, float tol, int32_t* list,
                                int32_t* n_out, void* stream) {
    if (int rc = check_frame(H, W, "nmf_accum_active: H or W below 1", "nmf_accum_active: more than 2^31 - 1 pixels")) return rc;
    NMF_REQUIRE(min_spp >= 0 && max_spp >= min_spp, NMF_EINVAL, "nmf_accum_active: 0 <= min_spp <= max_spp is required");
    NMF_REQUIRE(tol >= 0.f, NMF_EINVAL, "nmf_accum_active: tol must be 0 or above (not a NaN)");
    NMF_REQUIRE(state && list && n_out, NMF_EINVAL, "nmf_accum_active: null pointer");
    NMF_REQUIRE(((uintptr_t)state & 3) == 0, NMF_EINVAL, "nmf_accum_active: state must be 4-byte aligned");
    const int64_t P = (int64_t)H * W, n_tiles = cdiv(P, ACC_BLOCK);
    const float* st = static_cast<const float*>(state);
    int32_t* tiles = static_cast<int32_t*>(state) + (int64_t)NMF_ACCUM_PLANES * P;
    hipStream_t s = (hipStream_t)stream;
    NMF_LAUNCH(k_active_count, dim3((unsigned)n_tiles), dim3(ACC_BLOCK), 0, s, st, P, min_spp, max_spp, tol, tiles);
    NMF_LAUNCH(k_active_scan, dim3(1), dim3(ACC_BLOCK), 0, s, tiles, n_tiles, n_out);
    NMF_LAUNCH(k_active_emit, dim3((unsigned)n_tiles), dim3(ACC_BLOCK), 0, s, st, P, min_spp, max_spp, tol, (const int32_t*)tiles, list);
    NMF_CHECK_LAUNCH("nmf_accum_active");
    return NMF_OK;
}

extern "C" int nmf_accum_resolve(const void* state, int32_t H, int32_t W, float bg_r, float bg_g, float bg_b, int32_t tonemap,
                                 int32_t noclip, float* rgb_map, float* acc, float* depth, float* normal, float* se, float* count,
                                 void* stream) {
    if (int rc = check_frame(H, W, "nmf_accum_resolve: H or W below 1", "nmf_accum_resolve: more than 2^31 - 1 pixels")) return rc;
    NMF_REQUIRE(finite_f(bg_r) && finite_f(bg_g) && finite_f(bg_b), NMF_EINVAL, "nmf_accum_resolve: bg must be finite");
    NMF_REQUIRE(state, NMF_EINVAL, "nmf_accum_resolve: null state");
    NMF_REQUIRE(rgb_map || acc || depth || normal || se || count, NMF_EINVAL, "nmf_accum_resolve: no output (all six are null)");
    ResolveArgs A;
    A.state = static_cast<const float*>(state); A.P = (int64_t)H * W;
    A.bg[0] = bg_r; A.bg[1] = bg_g; A.bg[2] = bg_b; A.tonemap = tonemap; A.noclip = noclip;
    A.rgb_map = rgb_map; A.acc = acc; A.depth = depth; A.normal = normal; A.se = se; A.count = count;
    NMF_LAUNCH(k_accum_resolve, dim3((unsigned)cdiv(A.P, ACC_BLOCK)), dim3(ACC_BLOCK), 0, (hipStream_t)stream, A);
    NMF_CHECK_LAUNCH("nmf_accum_resolve");
    return NMF_OK;
}
