// Resampling of a spherical radiance function into the texel grid of an IntegralEquirect map under a rotation: relighting with a
// rotated environment and the direct import of a panorama (nmf_amd/relight.py).  The reference rotates its lights in
// notebooks (scripts/car_rotating_lights.ipynb) and imports a panorama by fitting the map to it (scripts/pano2cube.py); neither has a
// resampling kernel.
//
// Conventions (the lookup of env.hip, restated):  a direction d = (a, b, c) has the coordinates
//     cx = (atan2(b, a) mod 2 pi - pi) / pi,   cy = -2 atan2(c, hypot(a, b)) / pi        in [-1, 1]
// and back  phi = pi (cx + 1), theta = -pi cy / 2, d = (cos theta cos phi, cos theta sin phi, sin theta).  The summed-area table is an
// inclusive prefix sum sampled with align_corners at ix = (cx + 1)(W - 1) / 2, so texel column j covers ix in (j - 1, j] and its centre
// is at ix = j - 1/2; columns 1..W-1 cover 2 pi periodically (column 0 never enters a box), rows 1..H-1 the latitudes, and rows 0 and
// H - 1 also feed the pole colours through their means.
//
// One thread per destination texel; S x S stratified sub-samples of its extent, each turned into a direction, rotated by R^T
// (lighting rotated by R: L'(d) = L(R^T d)), looked up bilinearly in the source and averaged in a fixed order: no atomics, the same
// bytes on every run.  ALU-bound (a sincos pair, two atan2 and four taps per sub-sample) on a cache-resident source: no LDS staging.
// The arithmetic order below is restated in numpy by tests/test_relight_cpu.py (resample_np); contraction is off so that the fp32
// restatement and the kernel differ by the transcendental functions only.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr float RS_PI = 3.14159265358979323846f;
constexpr float RS_TWO_PI = 6.28318530717958647692f;

struct Rot3 {
    float m[9];   // row-major R
};

struct ResampleArgs {
    const float* src;
    int kind, Hs, Ws;
    Rot3 R;
    float gain;
    int S;
    float* dst;
    int H, W;
};

__device__ __forceinline__ int wrap_mod(int j, int P) {
    j %= P;
    return j < 0 ? j + P : j;
}

__global__ void __launch_bounds__(256) k_env_resample(ResampleArgs A) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_dst = (int64_t)A.H * A.W;
    if (t >= n_dst) return;
    const int i = (int)(t / A.W), j = (int)(t % A.W);
    const int S = A.S, Hs = A.Hs, Ws = A.Ws;
    const float sx = 2.f / (float)(A.W - 1), sy = 2.f / (float)(A.H - 1);
    const float hx = (float)(Ws - 1) * 0.5f, hy = (float)(Hs - 1) * 0.5f;
    const int64_t plane = (int64_t)Hs * Ws;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int a = 0; a < S; ++a) {
        const float fa = ((float)a + 0.5f) / (float)S;
        float cy = ((float)(i - 1) + fa) * sy - 1.f;
        cy = fminf(fmaxf(cy, -1.f), 1.f);
        const float th = (-RS_PI * cy) * 0.5f;
        float st, ct;
        sincosf(th, &st, &ct);
        for (int b = 0; b < S; ++b) {
            const float fb = ((float)b + 0.5f) / (float)S;
            const float cx = ((float)(j - 1) + fb) * sx - 1.f;
            const float ph = RS_PI * (cx + 1.f);
            float sp, cp;
            sincosf(ph, &sp, &cp);
            const float d0 = ct * cp, d1 = ct * sp, d2 = st;
            // s = R^T d
            const float s0 = (A.R.m[0] * d0 + A.R.m[3] * d1) + A.R.m[6] * d2;
            const float s1 = (A.R.m[1] * d0 + A.R.m[4] * d1) + A.R.m[7] * d2;
            const float s2 = (A.R.m[2] * d0 + A.R.m[5] * d1) + A.R.m[8] * d2;
            const float phi = atan2f(s1, s0);
            const float m = phi < 0.f ? phi + RS_TWO_PI : phi;
            const float scx = (m - RS_PI) / RS_PI;
            const float theta = atan2f(s2, sqrtf(s0 * s0 + s1 * s1));
            const float scy = ((-theta) / RS_PI) * 2.f;
            float u, v;
            int c0, c1, r0, r1;
            if (A.kind == 0) {
                // module map: texel centres at ix = j - 1/2; columns periodic over 1..Ws-1, rows clamped to 1..Hs-1
                u = (scx + 1.f) * hx + 0.5f;
                v = (scy + 1.f) * hy + 0.5f;
                const float fu = floorf(u), fv = floorf(v);
                const int ju = (int)fu, iv = (int)fv;
                u -= fu; v -= fv;
                c0 = wrap_mod(ju - 1, Ws - 1) + 1;
                c1 = wrap_mod(ju, Ws - 1) + 1;
                r0 = min(max(iv, 1), Hs - 1);
                r1 = min(max(iv + 1, 1), Hs - 1);
            } else {
                // panorama (pano2env.pixel_directions): row = (scy + 1)(Hp - 1) / 2, col = -scx (Wp - 1) / 2 mod (Wp - 1)
                u = (-scx * 0.5f) * (float)(Ws - 1);
                v = (scy + 1.f) * hy;
                const float fu = floorf(u), fv = floorf(v);
                const int ju = (int)fu, iv = (int)fv;
                u -= fu; v -= fv;
                c0 = wrap_mod(ju, Ws - 1);
                c1 = wrap_mod(ju + 1, Ws - 1);
                r0 = min(max(iv, 0), Hs - 1);
                r1 = min(max(iv + 1, 0), Hs - 1);
            }
            const float e = 1.f - u, s = 1.f - v;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float t00, t01, t10, t11;
                if (A.kind == 0) {
                    const float* p = A.src + c * plane;
                    t00 = p[(int64_t)r0 * Ws + c0]; t01 = p[(int64_t)r0 * Ws + c1];
                    t10 = p[(int64_t)r1 * Ws + c0]; t11 = p[(int64_t)r1 * Ws + c1];
                } else {
                    t00 = A.src[((int64_t)r0 * Ws + c0) * 3 + c]; t01 = A.src[((int64_t)r0 * Ws + c1) * 3 + c];
                    t10 = A.src[((int64_t)r1 * Ws + c0) * 3 + c]; t11 = A.src[((int64_t)r1 * Ws + c1) * 3 + c];
                }
                acc[c] = acc[c] + (s * (e * t00 + u * t01) + v * (e * t10 + u * t11));
            }
        }
    }
    const float inv = (float)(S * S);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float val = (acc[c] / inv) * A.gain;
        A.dst[c * n_dst + t] = logf(fmaxf(val, 1e-8f));      // fmaxf drops a NaN: the floor
    }
}

}  // namespace

extern "C" int nmf_env_resample(const float* src, int32_t kind, int32_t Hs, int32_t Ws, float r00, float r01, float r02, float r10,
                                float r11, float r12, float r20, float r21, float r22, float gain, int32_t supersample, float* dst,
                                int32_t H, int32_t W, void* stream) {
    NMF_REQUIRE(src && dst, NMF_EINVAL, "nmf_env_resample: null pointer");
    NMF_REQUIRE(Hs >= 4 && Ws >= 4 && H >= 4 && W >= 4, NMF_EINVAL, "nmf_env_resample: a size below 4");
    NMF_REQUIRE(supersample >= 1 && supersample <= 8, NMF_ERANGE, "nmf_env_resample: supersample outside 1..8");
    NMF_REQUIRE(kind == 0 || kind == 1, NMF_EINVAL, "nmf_env_resample: kind must be 0 (module map) or 1 (panorama)");
    NMF_REQUIRE(gain > 0.f && gain <= 3.4028235e38f, NMF_EINVAL, "nmf_env_resample: gain must be finite and positive");
    ResampleArgs A;
    const float R[9] = {r00, r01, r02, r10, r11, r12, r20, r21, r22};
    bool orthonormal = true;
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) {
            float g = 0.f;
            for (int k = 0; k < 3; ++k) g += R[3 * k + p] * R[3 * k + q];
            if (!(fabsf(g - (p == q ? 1.f : 0.f)) <= 1e-4f)) orthonormal = false;          // (a NaN fails too)
        }
    NMF_REQUIRE(orthonormal, NMF_EINVAL, "nmf_env_resample: R is not a rotation (max|R^T R - I| > 1e-4)");
    for (int k = 0; k < 9; ++k) A.R.m[k] = R[k];
    A.src = src; A.kind = kind; A.Hs = Hs; A.Ws = Ws; A.gain = gain; A.S = supersample; A.dst = dst; A.H = H; A.W = W;
    NMF_LAUNCH(k_env_resample, dim3((unsigned)cdiv((int64_t)H * W, 256)), dim3(256), 0, (hipStream_t)stream, A);
    NMF_CHECK_LAUNCH("nmf_env_resample");
    return NMF_OK;
}
