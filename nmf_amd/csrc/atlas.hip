// The two kernels of the texture bake of an exported mesh (nmf_amd/mesh.py:bake_textures): where every texel of a
// per-triangle atlas lies in the world, and the baked attributes of a chunk of texels as the bytes of the four texture planes.  The
// field queries between the two are the renderer's own (mesh.vertex_attributes).  The reference exports no textures.
//
// Both are restated in numpy fp32 by the tests (tests/test_atlas_cpu.py: atlas_numpy) and compared bit for bit (positions) and byte
// for byte (planes): contraction is off and '/' is hipcc's correctly rounded fp32 division, as in camera.hip; powf differs from the
// host's by ulps, which the store's test keeps away from a byte boundary by its choice of inputs.
#include "common.hpp"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int ATLAS_W_MIN = 4, ATLAS_W_MAX = 16384;

struct TexelArgs {
    const float* verts;        // [V][3]
    const int32_t* faces;      // [F][3]
    int64_t V, F;
    uint32_t W, T, nsq;        // nsq = W / T squares per row
    float b;                   // T - 3
    int64_t t0, n;
    float* pos;                // [n][3]
    int32_t* face_of;          // [n]
};

// One lane per texel, closed form (include/nmf_hip.h states the layout).  W^2 <= 2^28: 32-bit divisions.
__global__ void __launch_bounds__(256) k_atlas_texels(TexelArgs A) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n) return;
    const uint32_t t = (uint32_t)(A.t0 + k);
    const uint32_t y = t / A.W, x = t - y * A.W;
    const uint32_t cx = x / A.T, cy = y / A.T;
    int32_t face = -1;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    if (cx < A.nsq && cy < A.nsq) {
        uint32_t i = x - cx * A.T, j = y - cy * A.T;
        int64_t f = 2 * (int64_t)(cy * A.nsq + cx);
        if (i + j > A.T - 2) {                                     // the upper face: the same chart under the point mirror of the square
            f += 1;
            i = A.T - 1 - i;
            j = A.T - 1 - j;
        }
        if (f < A.F) {
            const int64_t a = A.faces[3 * f], b = A.faces[3 * f + 1], c = A.faces[3 * f + 2];
            if (a >= 0 && a < A.V && b >= 0 && b < A.V && c >= 0 && c < A.V) {      // (a caller error otherwise: the texel stays unowned)
                const float b1 = (float)i / A.b, b2 = (float)j / A.b;
                const float b0 = (1.f - b1) - b2;
                const float *va = A.verts + 3 * a, *vb = A.verts + 3 * b, *vc = A.verts + 3 * c;
                p0 = (b0 * va[0] + b1 * vb[0]) + b2 * vc[0];
                p1 = (b0 * va[1] + b1 * vb[1]) + b2 * vc[1];
                p2 = (b0 * va[2] + b1 * vb[2]) + b2 * vc[2];
                face = (int32_t)f;
            }
        }
    }
    A.face_of[k] = face;
    A.pos[3 * k] = p0;
    A.pos[3 * k + 1] = p1;
    A.pos[3 * k + 2] = p2;
}

struct StoreArgs {
    const int32_t* face_of;                          // [n], indexed by t - t0
    const float *albedo, *f0, *rough, *normal;
    int64_t t0, t1;                                  // the texels [t0, t1)
    uint8_t *albedo_tex, *f0_tex, *rough_tex, *normal_tex;
    int aligned;                                     // bit p: plane p (albedo, f0, rough, normal) is 4-byte aligned
};

__device__ __forceinline__ float nan0(float v) { return v != v ? 0.f : v; }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

constexpr float SRGB_LIMIT = 0.0031308f;
__device__ __forceinline__ float srgb(float x) {                 // modules/tonemap.py: the limit is also the floor under the power
    return x > SRGB_LIMIT ? 1.055f * powf(fmaxf(x, SRGB_LIMIT), 1.0f / 2.4f) - 0.055f : 12.92f * x;
}

enum { Q_SRGB = 0, Q_UNIT = 1, Q_NORMAL = 2 };

template <int MODE>
__device__ __forceinline__ uint32_t quantise(float v) {
    v = nan0(v);
    if (MODE == Q_SRGB) return (uint32_t)(uint8_t)(clamp01(srgb(v)) * 255.f);
    if (MODE == Q_UNIT) return (uint32_t)(uint8_t)(clamp01(v) * 255.f);
    return (uint32_t)(uint8_t)fminf(fmaxf(v * 127.f + 128.f, 0.f), 255.f);
}

// The three bytes of one texel in the low 24 bits, the first channel lowest; `src` is read for owned texels only.
template <int MODE>
__device__ __forceinline__ uint32_t texel_rgb(const float* src, int64_t k, bool owned) {
    if (!owned) return MODE == Q_NORMAL ? 0x808080u : 0u;
    return quantise<MODE>(src[3 * k]) | (quantise<MODE>(src[3 * k + 1]) << 8) | (quantise<MODE>(src[3 * k + 2]) << 16);
}

// The texels q0 + lo .. q0 + hi - 1 of a three-channel plane: 12 bytes as three dwords for a whole group of an aligned plane.
template <int MODE>
__device__ __forceinline__ void store_rgb(uint8_t* plane, const float* src, const StoreArgs& A, int64_t q0, int lo, int hi, uint32_t owned,
                                          bool dwords) {
    uint32_t v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (e >= lo && e < hi) ? texel_rgb<MODE>(src, q0 + e - A.t0, (owned >> e) & 1u) : 0u;
    if (dwords) {
        uint32_t* o = reinterpret_cast<uint32_t*>(plane + q0 * 3);
        o[0] = v[0] | (v[1] << 24);
        o[1] = (v[1] >> 8) | (v[2] << 16);
        o[2] = (v[2] >> 16) | (v[3] << 8);
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {                    // (unrolled with constant indices: v stays in registers)
        if (e < lo || e >= hi) continue;
        uint8_t* o = plane + (q0 + e) * 3;
        o[0] = (uint8_t)v[e];
        o[1] = (uint8_t)(v[e] >> 8);
        o[2] = (uint8_t)(v[e] >> 16);
    }
}

// One lane owns the group of four texels 4 g .. 4 g + 3 (global texel indices, so that a group's bytes are whole dwords of an aligned
// plane whatever t0 is); the groups at the two ends of [t0, t1) may be partial and store bytes.
__global__ void __launch_bounds__(256) k_atlas_store(StoreArgs A, int64_t g0, int64_t n_groups) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_groups) return;
    const int64_t q0 = (g0 + l) * 4;
    const int lo = q0 < A.t0 ? (int)(A.t0 - q0) : 0;
    const int hi = q0 + 4 > A.t1 ? (int)(A.t1 - q0) : 4;
    if (lo >= hi) return;
    const bool whole = hi - lo == 4;
    uint32_t owned = 0;
    for (int e = lo; e < hi; ++e) owned |= (A.face_of[q0 + e - A.t0] >= 0 ? 1u : 0u) << e;
    if (A.albedo_tex) store_rgb<Q_SRGB>(A.albedo_tex, A.albedo, A, q0, lo, hi, owned, whole && (A.aligned & 1));
    if (A.f0_tex) store_rgb<Q_UNIT>(A.f0_tex, A.f0, A, q0, lo, hi, owned, whole && (A.aligned & 2));
    if (A.normal_tex) store_rgb<Q_NORMAL>(A.normal_tex, A.normal, A, q0, lo, hi, owned, whole && (A.aligned & 8));
    if (A.rough_tex) {
        uint32_t v = 0;
        for (int e = lo; e < hi; ++e)
            if ((owned >> e) & 1u) v |= quantise<Q_UNIT>(A.rough[q0 + e - A.t0]) << (8 * e);
        if (whole && (A.aligned & 4)) {
            *reinterpret_cast<uint32_t*>(A.rough_tex + q0) = v;
        } else {
            for (int e = lo; e < hi; ++e) A.rough_tex[q0 + e] = (uint8_t)(v >> (8 * e));
        }
    }
}

}  // namespace

extern "C" int nmf_atlas_texels(const float* verts, const int32_t* faces, int64_t V, int64_t F, int32_t W, int32_t T, int64_t t0,
                                int64_t n, float* pos, int32_t* face_of, void* stream) {
    // (the sizes first, the pointers last: a refused call names what is wrong with it whatever the pointers are)
    NMF_REQUIRE(V >= 0 && F >= 0, NMF_EINVAL, "nmf_atlas_texels: V or F below 0");
    NMF_REQUIRE(W >= ATLAS_W_MIN && W <= ATLAS_W_MAX, NMF_EINVAL, "nmf_atlas_texels: W outside 4..16384");
    NMF_REQUIRE(T >= 4 && T <= W, NMF_EINVAL, "nmf_atlas_texels: T below 4 or above W");
    const int64_t nsq = W / T;
    NMF_REQUIRE(nsq * nsq >= (F + 1) / 2, NMF_EINVAL, "nmf_atlas_texels: (W / T)^2 squares do not hold F faces, two each");
    NMF_REQUIRE(n >= 0 && t0 >= 0 && t0 <= (int64_t)W * W && n <= (int64_t)W * W - t0, NMF_EINVAL,
                "nmf_atlas_texels: the texel range leaves [0, W^2]");
    NMF_REQUIRE(F == 0 || (verts && faces), NMF_EINVAL, "nmf_atlas_texels: null verts or faces");
    NMF_REQUIRE(n == 0 || (pos && face_of), NMF_EINVAL, "nmf_atlas_texels: null output");
    if (n == 0) return NMF_OK;
    TexelArgs A;
    A.verts = verts; A.faces = faces; A.V = V; A.F = F;
    A.W = (uint32_t)W; A.T = (uint32_t)T; A.nsq = (uint32_t)nsq; A.b = (float)(T - 3);
    A.t0 = t0; A.n = n; A.pos = pos; A.face_of = face_of;
    NMF_LAUNCH(k_atlas_texels, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, A);
    NMF_CHECK_LAUNCH("nmf_atlas_texels");
    return NMF_OK;
}

extern "C" int nmf_atlas_store(const int32_t* face_of, const float* albedo, const float* f0, const float* roughness, const float* normal,
                               int64_t t0, int64_t n, int32_t W, uint8_t* albedo_tex, uint8_t* f0_tex, uint8_t* rough_tex,
                               uint8_t* normal_tex, void* stream) {
    NMF_REQUIRE(W >= ATLAS_W_MIN && W <= ATLAS_W_MAX, NMF_EINVAL, "nmf_atlas_store: W outside 4..16384");
    NMF_REQUIRE(n >= 0 && t0 >= 0 && t0 <= (int64_t)W * W && n <= (int64_t)W * W - t0, NMF_EINVAL,
                "nmf_atlas_store: the texel range leaves [0, W^2]");
    NMF_REQUIRE(n == 0 || face_of, NMF_EINVAL, "nmf_atlas_store: null face_of");
    NMF_REQUIRE(n == 0 || ((albedo || !albedo_tex) && (f0 || !f0_tex) && (roughness || !rough_tex) && (normal || !normal_tex)), NMF_EINVAL,
                "nmf_atlas_store: a plane without its input");
    if (n == 0 || !(albedo_tex || f0_tex || rough_tex || normal_tex)) return NMF_OK;
    StoreArgs A;
    A.face_of = face_of; A.albedo = albedo; A.f0 = f0; A.rough = roughness; A.normal = normal;
    A.t0 = t0; A.t1 = t0 + n;
    A.albedo_tex = albedo_tex; A.f0_tex = f0_tex; A.rough_tex = rough_tex; A.normal_tex = normal_tex;
    uint8_t* const planes[4] = {albedo_tex, f0_tex, rough_tex, normal_tex};
    A.aligned = 0;
    for (int p = 0; p < 4; ++p) A.aligned |= (((uintptr_t)planes[p] & 3) == 0 ? 1 : 0) << p;
    const int64_t g0 = t0 / 4, n_groups = cdiv(A.t1, 4) - g0;
    NMF_LAUNCH(k_atlas_store, dim3((unsigned)cdiv(n_groups, 256)), dim3(256), 0, (hipStream_t)stream, A, g0, n_groups);
    NMF_CHECK_LAUNCH("nmf_atlas_store");
    return NMF_OK;
}
