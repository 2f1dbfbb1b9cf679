// Scene composition: several trained objects rendered under one environment (nmf_amd/compose.py).  The reference
// puts one object onto another by hand (scripts/toaster_on_car.py over fields/listrf.py: a second sampler, densities by max, the
// material heads of one model for every object); here every object keeps its own sampler, field and shading model in its own frame,
// and only the two pieces of glue between them run in this file:
//
//   nmf_rays_place     rays between the world frame and an object's frame under a similarity x_w = s R x_l + c
//   nmf_merge_rank     where each sample of K per-ray depth-sorted lists goes in the merged, depth-sorted list (stable K-way merge)
//   nmf_merge_scatter  one object's per-sample rows written to those places
//
// One thread per ray / per sample, closed form: no atomics, no LDS, the same bytes on every run.  A thread of nmf_merge_rank walks
// at most 7 binary searches over the other lists' segments of its ray (tens to a few hundred entries, contiguous, L2-resident);
// neighbouring threads are neighbouring samples of the same ray and list, so their searches take the same turns almost always
// and their loads hit the same cache lines.  The arithmetic order is restated in numpy by tests/test_compose_cpu.py; contraction is
// off so that the restatement and the kernels differ by nothing.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

struct Sim3 {
    float R[9];   // row-major rotation, local -> world
    float c[3];
    float s;
};

__global__ void __launch_bounds__(256) k_rays_place(const float* __restrict__ in, float* __restrict__ out, int64_t B, Sim3 P,
                                                    int inverse, int identity) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B) return;
    const float* q = in + r * 6;
    float* w = out + r * 6;
    const float o0 = q[0], o1 = q[1], o2 = q[2], d0 = q[3], d1 = q[4], d2 = q[5];
    if (identity) {         // R = I, c = 0, s = 1 exactly: the input's bits (1 * -0 + 0 would turn a -0 into +0)
        w[0] = o0; w[1] = o1; w[2] = o2; w[3] = d0; w[4] = d1; w[5] = d2;
        return;
    }
    if (inverse) {          // o' = R^T (o - c) / s,  d' = R^T d
        const float t0 = o0 - P.c[0], t1 = o1 - P.c[1], t2 = o2 - P.c[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            w[i] = ((P.R[i] * t0 + P.R[3 + i] * t1) + P.R[6 + i] * t2) / P.s;
            w[3 + i] = (P.R[i] * d0 + P.R[3 + i] * d1) + P.R[6 + i] * d2;
        }
    } else {                // o' = s R o + c,  d' = R d
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            w[i] = P.s * ((P.R[3 * i] * o0 + P.R[3 * i + 1] * o1) + P.R[3 * i + 2] * o2) + P.c[i];
            w[3 + i] = (P.R[3 * i] * d0 + P.R[3 * i + 1] * d1) + P.R[3 * i + 2] * d2;
        }
    }
}

// max|R^T R - I| <= 1e-4 (the bound of nmf_env_resample); a NaN fails too
bool is_rotation(const float* R) {
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) {
            float g = 0.f;
            for (int k = 0; k < 3; ++k) g += R[3 * k + p] * R[3 * k + q];
            if (!(fabsf(g - (p == q ? 1.f : 0.f)) <= 1e-4f)) return false;
        }
    return true;
}

bool is_finite(float v) { return v >= -3.4028235e38f && v <= 3.4028235e38f; }

struct MergeArgs {
    const int64_t* offsets[NMF_MERGE_MAX_LISTS];
    const float* z[NMF_MERGE_MAX_LISTS];
    int64_t* dst[NMF_MERGE_MAX_LISTS];
    float scale[NMF_MERGE_MAX_LISTS];
    int64_t M[NMF_MERGE_MAX_LISTS];
    int64_t first[NMF_MERGE_MAX_LISTS + 1];   // thread t serves list k where first[k] <= t < first[k + 1]
    int K;
    int64_t B;
    int64_t* offsets_m;
};

__device__ __forceinline__ int64_t seg_bound(const int64_t* off, int64_t r, int64_t M) {
    const int64_t v = off[r];
    return v < 0 ? 0 : (v > M ? M : v);         // a list's offsets never index past its M entries, whatever they hold
}

__global__ void __launch_bounds__(256) k_merge_rank(MergeArgs A) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= A.B) {                             // offsets_m = sum_k offsets_k
        int64_t s = 0;
        for (int j = 0; j < A.K; ++j) s += seg_bound(A.offsets[j], t, A.M[j]);
        A.offsets_m[t] = s;
    }
    if (t >= A.first[A.K]) return;
    int k = 0;
    while (k + 1 < A.K && t >= A.first[k + 1]) ++k;
    const int64_t i = t - A.first[k];
    // the sample's ray: the last r with offsets_k[r] <= i (empty rays share their offset with the next one)
    const int64_t* off = A.offsets[k];
    int64_t lo = 0, hi = A.B;                   // invariant: off[lo] <= i, and off[hi] > i or hi == B
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    const int64_t r = lo;
    const float zw = A.scale[k] * A.z[k][i];
    int64_t own0 = seg_bound(off, r, A.M[k]);
    int64_t rank = i - own0;
    if (rank < 0) rank = 0;
    int64_t base = 0, room = 0;
    for (int j = 0; j < A.K; ++j) {
        const int64_t a = seg_bound(A.offsets[j], r, A.M[j]), b = seg_bound(A.offsets[j], r + 1, A.M[j]);
        base += a;
        room += b > a ? b - a : 0;
        if (j == k || b <= a) continue;
        // entries of list j that sort before this one: s_j z_j < zw, or equal and j < k
        const float sj = A.scale[j];
        const float* zj = A.z[j];
        int64_t l = a, h = b;
        while (l < h) {
            const int64_t m = (l + h) >> 1;
            const float v = sj * zj[m];
            const bool before = j < k ? (v <= zw) : (v < zw);
            if (before) l = m + 1; else h = m;
        }
        rank += l - a;
    }
    if (rank >= room) rank = room > 0 ? room - 1 : 0;      // (only lists that break the ordering contract get here)
    A.dst[k][i] = base + rank;
}

struct ScatterArgs {
    int64_t M, M_total;
    const int64_t* dst;
    const float *sigma, *dist, *z, *normal;
    const int32_t *ray_id, *inv;
    float ratio, scale;
    float R[9];
    int32_t part, row_base;
    float *sigma_m, *dist_m, *z_m, *normal_m;
    int32_t *ray_id_m, *part_m, *src_m, *inv_m;
};

__global__ void __launch_bounds__(256) k_merge_scatter(ScatterArgs A) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.M) return;
    const int64_t d = A.dst[i];
    if (d < 0 || d >= A.M_total) return;        // never a store outside the merged arrays
    if (A.sigma_m) A.sigma_m[d] = A.sigma[i] * A.ratio;
    if (A.dist_m) A.dist_m[d] = A.dist[i];
    if (A.z_m) A.z_m[d] = A.scale * A.z[i];
    if (A.normal_m) {
        const float n0 = A.normal[3 * i], n1 = A.normal[3 * i + 1], n2 = A.normal[3 * i + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            A.normal_m[3 * d + c] = (A.R[3 * c] * n0 + A.R[3 * c + 1] * n1) + A.R[3 * c + 2] * n2;
    }
    if (A.ray_id_m) A.ray_id_m[d] = A.ray_id[i];
    if (A.part_m) A.part_m[d] = A.part;
    if (A.src_m) A.src_m[d] = (int32_t)i;
    if (A.inv_m) {
        const int32_t v = A.inv[i];
        A.inv_m[d] = v >= 0 ? v + A.row_base : -1;
    }
}

}  // namespace

extern "C" int nmf_rays_place(const float* rays_in, const float* R, const float* c, float s, int32_t inverse, int64_t B,
                              float* rays_out, void* stream) {
    NMF_REQUIRE(R && c, NMF_EINVAL, "nmf_rays_place: null R or c");
    NMF_REQUIRE(B >= 0, NMF_EINVAL, "nmf_rays_place: B < 0");
    NMF_REQUIRE(B == 0 || (rays_in && rays_out), NMF_EINVAL, "nmf_rays_place: null pointer");
    NMF_REQUIRE(inverse == 0 || inverse == 1, NMF_EINVAL, "nmf_rays_place: inverse must be 0 or 1");
    NMF_REQUIRE(is_finite(s) && s > 0.f, NMF_EINVAL, "nmf_rays_place: s must be finite and positive");
    NMF_REQUIRE(is_finite(c[0]) && is_finite(c[1]) && is_finite(c[2]), NMF_EINVAL, "nmf_rays_place: c is not finite");
    NMF_REQUIRE(is_rotation(R), NMF_EINVAL, "nmf_rays_place: R is not a rotation (max|R^T R - I| > 1e-4)");
    NMF_REQUIRE(B <= 0x7fffffffLL * 256, NMF_ERANGE, "nmf_rays_place: too many rays");
    if (B == 0) return NMF_OK;
    Sim3 P;
    int identity = (s == 1.f);
    for (int k = 0; k < 9; ++k) {
        P.R[k] = R[k];
        identity &= (R[k] == ((k % 4 == 0) ? 1.f : 0.f));
    }
    for (int k = 0; k < 3; ++k) {
        P.c[k] = c[k];
        identity &= (c[k] == 0.f);
    }
    P.s = s;
    NMF_LAUNCH(k_rays_place, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, rays_in, rays_out, B, P, (int)inverse,
               identity);
    NMF_CHECK_LAUNCH("nmf_rays_place");
    return NMF_OK;
}

extern "C" int nmf_merge_rank(int32_t K, const nmf_merge_lists* lists, int64_t B, int64_t* offsets_m, void* stream) {
    NMF_REQUIRE(K >= 1 && K <= NMF_MERGE_MAX_LISTS, NMF_ERANGE, "nmf_merge_rank: K outside 1..8");
    NMF_REQUIRE(lists && offsets_m, NMF_EINVAL, "nmf_merge_rank: null pointer");
    NMF_REQUIRE(B >= 0, NMF_EINVAL, "nmf_merge_rank: B < 0");
    MergeArgs A;
    A.K = K; A.B = B; A.offsets_m = offsets_m;
    A.first[0] = 0;
    for (int k = 0; k < NMF_MERGE_MAX_LISTS; ++k) {
        const bool used = k < K;
        if (used) {
            NMF_REQUIRE(lists->M[k] >= 0, NMF_EINVAL, "nmf_merge_rank: a list with M < 0");
            NMF_REQUIRE(lists->offsets[k], NMF_EINVAL, "nmf_merge_rank: a list without offsets");
            NMF_REQUIRE(lists->M[k] == 0 || (lists->z[k] && lists->dst[k]), NMF_EINVAL, "nmf_merge_rank: null z or dst of a list with M > 0");
            NMF_REQUIRE(is_finite(lists->scale[k]) && lists->scale[k] > 0.f, NMF_EINVAL, "nmf_merge_rank: a scale must be finite and positive");
        }
        A.offsets[k] = used ? lists->offsets[k] : nullptr;
        A.z[k] = used ? lists->z[k] : nullptr;
        A.dst[k] = used ? lists->dst[k] : nullptr;
        A.scale[k] = used ? lists->scale[k] : 1.f;
        A.M[k] = used ? lists->M[k] : 0;
        A.first[k + 1] = A.first[k] + A.M[k];
    }
    NMF_REQUIRE(B > 0 || A.first[K] == 0, NMF_EINVAL, "nmf_merge_rank: samples without rays");
    const int64_t threads = A.first[K] > B + 1 ? A.first[K] : B + 1;
    NMF_REQUIRE(threads <= 0x7fffffffLL * 256, NMF_ERANGE, "nmf_merge_rank: too many samples");
    NMF_LAUNCH(k_merge_rank, dim3((unsigned)cdiv(threads, 256)), dim3(256), 0, (hipStream_t)stream, A);
    NMF_CHECK_LAUNCH("nmf_merge_rank");
    return NMF_OK;
}

extern "C" int nmf_merge_scatter(int64_t M_k, int64_t M_total, const int64_t* dst, const float* sigma, const float* dist, const float* z,
                                 const float* normal, const int32_t* ray_id, const int32_t* inv, float sigma_ratio, float scale,
                                 const float* R, int32_t part, int64_t row_base, float* sigma_m, float* dist_m, float* z_m,
                                 float* normal_m, int32_t* ray_id_m, int32_t* part_m, int32_t* src_m, int32_t* inv_m, void* stream) {
    NMF_REQUIRE(M_k >= 0 && M_total >= M_k, NMF_EINVAL, "nmf_merge_scatter: M_k < 0 or M_total < M_k");
    NMF_REQUIRE(part >= 0 && part < NMF_MERGE_MAX_LISTS, NMF_ERANGE, "nmf_merge_scatter: part outside 0..7");
    NMF_REQUIRE(M_k <= 0x7fffffffLL && row_base >= 0 && row_base <= 0x7fffffffLL, NMF_ERANGE, "nmf_merge_scatter: M_k or row_base above 2^31 - 1");
    NMF_REQUIRE(is_finite(sigma_ratio) && sigma_ratio > 0.f && is_finite(scale) && scale > 0.f, NMF_EINVAL,
                "nmf_merge_scatter: sigma_ratio and scale must be finite and positive");
    NMF_REQUIRE(!normal_m || (R && is_rotation(R)), NMF_EINVAL, "nmf_merge_scatter: R is null or not a rotation (max|R^T R - I| > 1e-4)");
    if (M_k == 0) return NMF_OK;
    NMF_REQUIRE(dst, NMF_EINVAL, "nmf_merge_scatter: null dst");
    NMF_REQUIRE((!sigma_m || sigma) && (!dist_m || dist) && (!z_m || z) && (!normal_m || normal) && (!ray_id_m || ray_id) && (!inv_m || inv),
                NMF_EINVAL, "nmf_merge_scatter: an output without its input");
    ScatterArgs A;
    A.M = M_k; A.M_total = M_total; A.dst = dst;
    A.sigma = sigma; A.dist = dist; A.z = z; A.normal = normal; A.ray_id = ray_id; A.inv = inv;
    A.ratio = sigma_ratio; A.scale = scale;
    for (int k = 0; k < 9; ++k) A.R[k] = (normal_m && R) ? R[k] : 0.f;
    A.part = part; A.row_base = (int32_t)row_base;
    A.sigma_m = sigma_m; A.dist_m = dist_m; A.z_m = z_m; A.normal_m = normal_m;
    A.ray_id_m = ray_id_m; A.part_m = part_m; A.src_m = src_m; A.inv_m = inv_m;
    NMF_LAUNCH(k_merge_scatter, dim3((unsigned)cdiv(M_k, 256)), dim3(256), 0, (hipStream_t)stream, A);
    NMF_CHECK_LAUNCH("nmf_merge_scatter");
    return NMF_OK;
}
