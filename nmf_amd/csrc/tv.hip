// Total-variation regularisers of the training step for gfx950 (reference: utils.py:139-151 TVLoss on the VM planes and lines,
// modules/integral_equirect.py:399-407 tv_loss on the environment map; applied per chunk by train.py:684-709).  The reference
// runs about twenty elementwise launches with plane-sized temporaries per tensor and direction; here the weighted value AND the
// weighted gradient of up to 16 tensors are ONE launch.
//
// Every term is the reference's expression restated in fp32, operation by operation (this file is compiled with
// -ffp-contract=off: no a*b+c -> fma), the value is the fp64 sum of the fp32 terms.
//   plane  x[C][H][W], W > 1:  t(c,h,w) = sqrt(dw^2 + dh^2 + 1e-5), dw = x[h][w+1] - x[h][w], dh = x[h+1][w] - x[h][w], h < H-1, w < W-1
//   line   x[C][G][1]:         t(c,g)   = |x[g+1] - x[g]|,                                                              g < G-1
//   envmap x[3][H][W]:         t(c,h,w) = |a| + |b| + 1e-8, a = x[c+1][h][w] - x[c][h][w], b = x[c][h+1][w] - x[c][h][w],  c < 2, h < H-1
//          (the reference slices bg_mat[0] = [3][H][W] as if it were [H][W][3]: "tv_h" is the difference of adjacent CHANNELS)
// value = scale * sum_i w_i * mean(t_i);  g_i += (scale * w_i / n_terms_i) * d(sum t_i)/dx_i.
//
// Gradient in GATHER form: a thread owns elements of x, evaluates its own term and the (at most two) terms of its lower-index
// neighbours that contain its element, and adds the three contributions to its elements of g -- no atomics, one read-modify-write
// of g.  Neighbour values come from the cache hierarchy: the tensors are stored channel-last ([H][W][C], C = 16 / 24), so the
// "left" neighbour of a lane is C floats away and the row above W*C floats -- neither is a neighbouring lane (no shuffle), and
// a workgroup's 1024 consecutive elements touch 7 shifted copies of the same few lines (L1 / L2 hits); an LDS tile would stage
// each element once to save reads that never leave the CU's cache.
//
// Value: every workgroup leaves the fp64 sum of its terms (already weighted by w_i / n_terms_i) in the workspace with a
// write-through store and draws a ticket; the workgroup that draws the last one adds the partial sums in workgroup order and WRITES
// the value (no zero fill, no float atomics: the same bits on every run and stream), then resets the ticket.
#include "common.hpp"

namespace {

constexpr int TV_MAX = 16;
constexpr int TV_THREADS = 256;
constexpr int TV_ITEMS = 4;                       // elements per thread, strided by the workgroup size (coalesced)
constexpr int TV_BLOCK_ELEMS = TV_THREADS * TV_ITEMS;

struct TvTab {
    const float* x[TV_MAX];
    float* g[TV_MAX];
    int32_t dim[TV_MAX][3];      // C, H, W
    int32_t xs[TV_MAX][3];       // element strides of x along C, H, W
    int32_t gs[TV_MAX][3];       // ... of g
    int32_t kind[TV_MAX];
    int32_t chan_fast[TV_MAX];   // 1: consecutive elements of the launch walk the channels first (channel-last storage)
    float w[TV_MAX];
    float n_terms[TV_MAX];
    uint32_t blk0[TV_MAX + 1];   // first workgroup of tensor i
    int32_t count;
};

__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// own term + the gradient of sum(t) with respect to element (c, h, w)
struct TvView {
    const float* __restrict__ x;
    int sc, sh, sw;
    __device__ __forceinline__ float at(int c, int h, int w) const { return x[(int64_t)c * sc + (int64_t)h * sh + (int64_t)w * sw]; }
};

__device__ __forceinline__ void plane_elem(const TvView& v, int H, int W, int c, int h, int w, float& term, float& grad) {
    const float a = v.at(c, h, w);
    float own = 0.f, left = 0.f, up = 0.f;
    term = 0.f;
    if (h < H - 1 && w < W - 1) {
        const float dw = v.at(c, h, w + 1) - a, dh = v.at(c, h + 1, w) - a;
        const float t = sqrtf(dw * dw + dh * dh + 1e-5f);
        term = t;
        own = 0.f - dw / t - dh / t;
    }
    if (w >= 1 && h < H - 1) {                   // term (h, w-1): this element is its x[h][w+1]
        const float b = v.at(c, h, w - 1);
        const float dw = a - b, dh = v.at(c, h + 1, w - 1) - b;
        left = dw / sqrtf(dw * dw + dh * dh + 1e-5f);
    }
    if (h >= 1 && w < W - 1) {                   // term (h-1, w): this element is its x[h+1][w]
        const float b = v.at(c, h - 1, w);
        const float dw = v.at(c, h - 1, w + 1) - b, dh = a - b;
        up = dh / sqrtf(dw * dw + dh * dh + 1e-5f);
    }
    grad = own + left + up;
}

__device__ __forceinline__ void line_elem(const TvView& v, int G, int c, int g, float& term, float& grad) {
    const float a = v.at(c, g, 0);
    float own = 0.f, prev = 0.f;
    term = 0.f;
    if (g < G - 1) {
        const float d = v.at(c, g + 1, 0) - a;
        term = fabsf(d);
        own = 0.f - sgn(d);
    }
    if (g >= 1) prev = sgn(a - v.at(c, g - 1, 0));
    grad = own + prev;
}

__device__ __forceinline__ void env_elem(const TvView& v, int C, int H, int c, int h, int w, float& term, float& grad) {
    const float a = v.at(c, h, w);
    float own = 0.f, chan = 0.f, row = 0.f;
    term = 0.f;
    if (c < C - 1 && h < H - 1) {
        const float da = v.at(c + 1, h, w) - a, db = v.at(c, h + 1, w) - a;
        term = fabsf(da) + fabsf(db) + 1e-8f;
        own = 0.f - sgn(da) - sgn(db);
    }
    if (c >= 1 && h < H - 1) chan = sgn(a - v.at(c - 1, h, w));      // term (c-1, h): this element is its x[c+1][h]
    if (c < C - 1 && h >= 1) row = sgn(a - v.at(c, h - 1, w));       // term (c, h-1): this element is its x[c][h+1]
    grad = own + chan + row;
}

__device__ __forceinline__ double block_sum_f64(double v, double* ws) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) ws[wid] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < TV_THREADS / 64; ++w) t += ws[w];
    __syncthreads();
    return t;   // valid on thread 0
}

__global__ void __launch_bounds__(TV_THREADS) k_tv_fwd_bwd(TvTab tab, const float* __restrict__ scale_dev, float* __restrict__ value_out,
                                                           int want_grad, uint32_t* ticket, unsigned long long* partial) {
    __shared__ double ws[TV_THREADS / 64 + 1];
    int i = 0;
    while (i + 1 < tab.count && blockIdx.x >= tab.blk0[i + 1]) ++i;
    const int C = tab.dim[i][0], H = tab.dim[i][1], W = tab.dim[i][2];
    const int kind = tab.kind[i];
    const int64_t n = (int64_t)C * H * W;
    const TvView v{tab.x[i], tab.xs[i][0], tab.xs[i][1], tab.xs[i][2]};
    float* __restrict__ g = tab.g[i];
    const int gc = tab.gs[i][0], gh = tab.gs[i][1], gw = tab.gs[i][2];
    const bool chan_fast = tab.chan_fast[i] != 0;
    const float scale = scale_dev[0];
    const float coef = scale * tab.w[i] / tab.n_terms[i];
    double acc = 0.0;
    const uint32_t n32 = (uint32_t)n;                 // (n <= 2^31 - 1: 32-bit index arithmetic)
    const uint32_t base = (blockIdx.x - tab.blk0[i]) * (uint32_t)TV_BLOCK_ELEMS + threadIdx.x;
#pragma unroll
    for (int k = 0; k < TV_ITEMS; ++k) {
        const uint32_t e = base + (uint32_t)(k * TV_THREADS);
        if (e >= n32) break;
        int c, h, w;
        if (chan_fast) {
            c = (int)(e % (uint32_t)C);
            const uint32_t r = e / (uint32_t)C;
            w = (int)(r % (uint32_t)W);
            h = (int)(r / (uint32_t)W);
        } else {
            w = (int)(e % (uint32_t)W);
            const uint32_t r = e / (uint32_t)W;
            h = (int)(r % (uint32_t)H);
            c = (int)(r / (uint32_t)H);
        }
        float term, grad;
        if (kind == NMF_TV_PLANE) plane_elem(v, H, W, c, h, w, term, grad);
        else if (kind == NMF_TV_LINE) line_elem(v, H, c, h, term, grad);
        else env_elem(v, C, H, c, h, w, term, grad);
        acc += (double)term;
        if (want_grad) {
            const int64_t o = (int64_t)c * gc + (int64_t)h * gh + (int64_t)w * gw;
            g[o] = g[o] + coef * grad;
        }
    }
    if (!value_out) return;
    const double t = block_sum_f64(acc, ws) * ((double)tab.w[i] / (double)tab.n_terms[i]);
    if (threadIdx.x == 0) {
        // write-through store of the partial sum, drained before the ticket: the last workgroup reads it with agent-scope loads
        __hip_atomic_store(partial + blockIdx.x, (unsigned long long)__double_as_longlong(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ws[TV_THREADS / 64] = drawn == gridDim.x - 1 ? 1.0 : 0.0;
    }
    __syncthreads();
    if (ws[TV_THREADS / 64] == 0.0) return;
    double a = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += TV_THREADS)
        a += __longlong_as_double((long long)__hip_atomic_load(partial + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    __syncthreads();
    const double total = block_sum_f64(a, ws);
    if (threadIdx.x == 0) {
        value_out[0] = (float)((double)scale * total);
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// shape / kind checks shared by the size query and the launch; -> number of workgroups, or a negative code
static int64_t tv_plan(const int32_t* shape, const int32_t* kind, int32_t count, TvTab* tab) {
    if (count > TV_MAX) return nmf_fail(NMF_ERANGE, "nmf_tv: at most 16 tensors");
    if (count < 1 || !shape || !kind) return nmf_fail(NMF_EINVAL, "nmf_tv: no tensor, or a null shape / kind table");
    int64_t blocks = 0;
    for (int i = 0; i < count; ++i) {
        const int64_t C = shape[3 * i], H = shape[3 * i + 1], W = shape[3 * i + 2];
        if (C < 1 || H < 1 || W < 1) return nmf_fail(NMF_EINVAL, "nmf_tv: a dimension below 1");
        if (C * H * W > (int64_t)0x7fffffff) return nmf_fail(NMF_ERANGE, "nmf_tv: a tensor of more than 2^31 - 1 elements");
        int64_t terms;
        switch (kind[i]) {
            case NMF_TV_PLANE:
                if (H < 2 || W < 2) return nmf_fail(NMF_ERANGE, "nmf_tv: a plane needs H >= 2 and W >= 2 (its mean is over an empty set)");
                terms = C * (H - 1) * (W - 1);
                break;
            case NMF_TV_LINE:
                if (W != 1) return nmf_fail(NMF_EINVAL, "nmf_tv: a line is [C][G][1]");
                if (H < 2) return nmf_fail(NMF_ERANGE, "nmf_tv: a line needs G >= 2 (its mean is over an empty set)");
                terms = C * (H - 1);
                break;
            case NMF_TV_ENVMAP:
                if (C != 3) return nmf_fail(NMF_EINVAL, "nmf_tv: an environment map is [3][H][W]");
                if (H < 2) return nmf_fail(NMF_ERANGE, "nmf_tv: an environment map needs H >= 2 (its mean is over an empty set)");
                terms = (C - 1) * (H - 1) * W;
                break;
            default:
                return nmf_fail(NMF_EINVAL, "nmf_tv: unknown kind");
        }
        if (tab) {
            tab->dim[i][0] = (int32_t)C; tab->dim[i][1] = (int32_t)H; tab->dim[i][2] = (int32_t)W;
            tab->kind[i] = kind[i];
            tab->n_terms[i] = (float)terms;
            tab->blk0[i] = (uint32_t)blocks;
        }
        blocks += cdiv(C * H * W, TV_BLOCK_ELEMS);
    }
    if (blocks > (int64_t)0x7fffffff) return nmf_fail(NMF_ERANGE, "nmf_tv: too many workgroups");
    if (tab) {
        for (int i = count; i <= TV_MAX; ++i) tab->blk0[i] = (uint32_t)blocks;
        tab->count = count;
    }
    return blocks;
}

// strides of a dense tensor: every element inside [0, numel), positive along every dimension longer than 1
static bool tv_strides(const int64_t* s, const int32_t dim[3], int32_t out[3]) {
    int64_t last = 0, numel = 1;
    for (int d = 0; d < 3; ++d) {
        const int64_t st = dim[d] > 1 ? s[d] : 0;
        if (st < 0 || st > (int64_t)0x7fffffff || (dim[d] > 1 && st < 1)) return false;
        last += st * (dim[d] - 1);
        numel *= dim[d];
        out[d] = (int32_t)st;
    }
    return last == numel - 1;
}

}  // namespace

extern "C" int64_t nmf_tv_workspace_bytes(const int32_t* shape, const int32_t* kind, int32_t count) {
    const int64_t blocks = tv_plan(shape, kind, count, nullptr);
    if (blocks < 0) return blocks;
    return 16 + 8 * blocks;
}

extern "C" int nmf_tv_fwd_bwd(const float* const x[], float* const g[], const int32_t* shape, const int64_t* x_stride,
                              const int64_t* g_stride, const int32_t* kind, const float w[], int32_t count, const float* scale_dev,
                              float* value_out, void* workspace, int64_t workspace_bytes, void* stream) {
    TvTab t;
    memset(&t, 0, sizeof(t));
    const int64_t blocks = tv_plan(shape, kind, count, &t);
    if (blocks < 0) return (int)blocks;
    NMF_REQUIRE(g || value_out, NMF_EINVAL, "nmf_tv_fwd_bwd: neither a gradient table nor a value output");
    NMF_REQUIRE(scale_dev && x && w && x_stride && (!g || g_stride), NMF_EINVAL, "nmf_tv_fwd_bwd: null");
    if (value_out)
        NMF_REQUIRE(workspace && workspace_bytes >= 16 + 8 * blocks && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                    NMF_EINVAL, "nmf_tv_fwd_bwd: workspace missing, too small or not 16-byte aligned");
    for (int i = 0; i < count; ++i) {
        NMF_REQUIRE(x[i] && (!g || g[i]), NMF_EINVAL, "nmf_tv_fwd_bwd: null tensor");
        NMF_REQUIRE(tv_strides(x_stride + 3 * i, t.dim[i], t.xs[i]), NMF_EINVAL, "nmf_tv_fwd_bwd: x is not a dense tensor of that shape");
        if (g) NMF_REQUIRE(tv_strides(g_stride + 3 * i, t.dim[i], t.gs[i]), NMF_EINVAL, "nmf_tv_fwd_bwd: g is not a dense tensor of that shape");
        NMF_REQUIRE(w[i] == w[i], NMF_EINVAL, "nmf_tv_fwd_bwd: a weight is NaN");
        t.x[i] = x[i];
        t.g[i] = g ? g[i] : nullptr;
        t.w[i] = w[i];
        t.chan_fast[i] = (t.dim[i][0] > 1 && t.xs[i][0] == 1) ? 1 : 0;
    }
    char* ws = value_out ? static_cast<char*>(workspace) : nullptr;
    NMF_LAUNCH(k_tv_fwd_bwd, dim3((unsigned)blocks), dim3(TV_THREADS), 0, (hipStream_t)stream, t, scale_dev, value_out, g ? 1 : 0,
               reinterpret_cast<uint32_t*>(ws), reinterpret_cast<unsigned long long*>(ws ? ws + 16 : nullptr));
    NMF_CHECK_LAUNCH("nmf_tv_fwd_bwd");
    return NMF_OK;
}
