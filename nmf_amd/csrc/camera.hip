// The two per-frame kernels around the evaluation pass when a camera path is rendered (nmf_amd/renderer.py:evaluation_path; DESIGN.md
// 10.7): the pixel rays of a pinhole camera formed on the device from its pose, and the finished 8-bit picture (rgb | depth | normal |
// acc panels side by side) formed on the device from the pass's float maps, so that a frame costs no ray upload and one uint8 read-back.
// The reference makes its rays on the host for every view of a data set (dataLoader/ray_utils.py:23-41,65-85) and quantises each map
// with numpy (renderer.py:343-347, 440-463; utils.visualize_depth_numpy).
//
// Both are restated in numpy fp32 by the tests (tests/test_camera_path_cpu.py: camera_rays_np, frame_finish_np) and compared bit for
// bit: contraction is off, and '/' and sqrtf are hipcc's correctly rounded fp32 forms (its default; the _rn intrinsics of the HIP
// headers map sqrt to the native instruction, which is not).
#include "common.hpp"

#include <math.h>

#pragma clang fp contract(off)

namespace {

struct CameraArgs {
    float r[9];        // row-major rotation of the camera-to-world matrix: uniform, read from SGPRs
    float t[3];
    float fx, fy, cx, cy;
    int W;
    int64_t P;
    float* rays;       // [P][6]
};

// One lane per pixel; its 24 contiguous bytes leave as three 8-byte stores (a row of 6 floats is 8-byte aligned, not 16).
__global__ void __launch_bounds__(256) k_camera_rays(CameraArgs A) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= A.P) return;
    const uint32_t row = (uint32_t)p / (uint32_t)A.W, col = (uint32_t)p - row * (uint32_t)A.W;      // P < 2^31: 32-bit division
    const float x = (((float)col + 0.5f) - A.cx) / A.fx;
    const float y = (((float)row + 0.5f) - A.cy) / A.fy;
    const float n = sqrtf((x * x + y * y) + 1.f);
    const float dx = x / n, dy = y / n, dz = 1.f / n;
    const float w0 = (A.r[0] * dx + A.r[1] * dy) + A.r[2] * dz;
    const float w1 = (A.r[3] * dx + A.r[4] * dy) + A.r[5] * dz;
    const float w2 = (A.r[6] * dx + A.r[7] * dy) + A.r[8] * dz;
    float2* o = reinterpret_cast<float2*>(A.rays + p * 6);
    o[0] = make_float2(A.t[0], A.t[1]);
    o[1] = make_float2(A.t[2], w0);
    o[2] = make_float2(w1, w2);
}

struct FinishArgs {
    const float *rgb, *depth, *normal, *acc;
    int o_rgb, o_depth, o_normal, o_acc;      // the panel each input fills (its ordinal among the non-null ones), -1: absent
    float near, range;                        // range = (far - near) + 1e-8f
    const uint8_t* lut;
    int W, n_panels;
    int64_t T;                                // output pixels: H n_panels W
    uint8_t* out;
};

inline bool finite_f(float v) { return fabsf(v) <= 3.4028235e38f; }      // (false for a NaN)

__device__ __forceinline__ float nan0(float v) { return v != v ? 0.f : v; }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// the three bytes of output pixel q (row-major over [H][n_panels W]) in the low 24 bits, red lowest
__device__ __forceinline__ uint32_t finish_pixel(const FinishArgs& A, int64_t q) {
    const uint32_t W = (uint32_t)A.W, stride = (uint32_t)A.n_panels * W;                             // T < 2^31: 32-bit divisions
    const uint32_t row = (uint32_t)q / stride, rem = (uint32_t)q - row * stride;
    const uint32_t kk = rem / W, col = rem - kk * W;
    const int k = (int)kk;
    const int64_t p = (int64_t)row * W + col;
    uint32_t b0, b1, b2;
    if (k == A.o_rgb) {
        b0 = (uint32_t)(uint8_t)(clamp01(nan0(A.rgb[p * 3 + 0])) * 255.f);
        b1 = (uint32_t)(uint8_t)(clamp01(nan0(A.rgb[p * 3 + 1])) * 255.f);
        b2 = (uint32_t)(uint8_t)(clamp01(nan0(A.rgb[p * 3 + 2])) * 255.f);
    } else if (k == A.o_depth) {
        const float t = clamp01((nan0(A.depth[p]) - A.near) / A.range);
        const uint32_t g = (uint32_t)(uint8_t)(255.f * t);
        if (A.lut) {
            b0 = A.lut[g * 3 + 0]; b1 = A.lut[g * 3 + 1]; b2 = A.lut[g * 3 + 2];
        } else {
            b0 = b1 = b2 = g;
        }
    } else if (k == A.o_normal) {
        b0 = (uint32_t)(uint8_t)fminf(fmaxf(nan0(A.normal[p * 3 + 0]) * 127.f + 128.f, 0.f), 255.f);
        b1 = (uint32_t)(uint8_t)fminf(fmaxf(nan0(A.normal[p * 3 + 1]) * 127.f + 128.f, 0.f), 255.f);
        b2 = (uint32_t)(uint8_t)fminf(fmaxf(nan0(A.normal[p * 3 + 2]) * 127.f + 128.f, 0.f), 255.f);
    } else {
        b0 = b1 = b2 = (uint32_t)(uint8_t)(255.f * clamp01(nan0(A.acc[p])));
    }
    return b0 | (b1 << 8) | (b2 << 16);
}

// One lane owns four consecutive output pixels: 12 bytes, three whole dwords (out 4-byte aligned, which the host checks once; the
// group index times 12 keeps the alignment).  The last lane of an image whose pixel count is no multiple of 4, and every lane of a
// misaligned `out`, store bytes.
__global__ void __launch_bounds__(256) k_frame_finish(FinishArgs A, int aligned) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t q0 = g * 4;
    if (q0 >= A.T) return;
    if (aligned && q0 + 4 <= A.T) {
        const uint32_t a = finish_pixel(A, q0), b = finish_pixel(A, q0 + 1), c = finish_pixel(A, q0 + 2), d = finish_pixel(A, q0 + 3);
        uint32_t* o = reinterpret_cast<uint32_t*>(A.out + q0 * 3);
        o[0] = a | (b << 24);
        o[1] = (b >> 8) | (c << 16);
        o[2] = (c >> 16) | (d << 8);
        return;
    }
    const int64_t q1 = q0 + 4 < A.T ? q0 + 4 : A.T;
    for (int64_t q = q0; q < q1; ++q) {
        const uint32_t v = finish_pixel(A, q);
        A.out[q * 3 + 0] = (uint8_t)v;
        A.out[q * 3 + 1] = (uint8_t)(v >> 8);
        A.out[q * 3 + 2] = (uint8_t)(v >> 16);
    }
}

}  // namespace

extern "C" int nmf_camera_rays(float r00, float r01, float r02, float r10, float r11, float r12, float r20, float r21, float r22,
                               float tx, float ty, float tz, float fx, float fy, float cx, float cy, int32_t H, int32_t W, float* rays,
                               void* stream) {
    // (the arguments first, the pointer last: a refused call names what is wrong with it whatever the pointers are)
    NMF_REQUIRE(H >= 1 && W >= 1, NMF_EINVAL, "nmf_camera_rays: H or W below 1");
    NMF_REQUIRE(finite_f(fx) && finite_f(fy) && fx != 0.f && fy != 0.f, NMF_EINVAL, "nmf_camera_rays: fx and fy must be finite and non-zero");
    const float pose[12] = {r00, r01, r02, r10, r11, r12, r20, r21, r22, tx, ty, tz};
    bool finite = finite_f(cx) && finite_f(cy);
    for (int k = 0; k < 12; ++k) finite = finite && finite_f(pose[k]);
    NMF_REQUIRE(finite, NMF_EINVAL, "nmf_camera_rays: the pose, cx and cy must be finite");
    NMF_REQUIRE((int64_t)H * W <= 2147483647LL, NMF_ERANGE, "nmf_camera_rays: more than 2^31 - 1 pixels");
    NMF_REQUIRE(rays, NMF_EINVAL, "nmf_camera_rays: null pointer");
    NMF_REQUIRE(((uintptr_t)rays & 7) == 0, NMF_EINVAL, "nmf_camera_rays: rays must be 8-byte aligned");
    CameraArgs A;
    for (int k = 0; k < 9; ++k) A.r[k] = pose[k];
    for (int k = 0; k < 3; ++k) A.t[k] = pose[9 + k];
    A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.W = W; A.P = (int64_t)H * W; A.rays = rays;
    NMF_LAUNCH(k_camera_rays, dim3((unsigned)cdiv(A.P, 256)), dim3(256), 0, (hipStream_t)stream, A);
    NMF_CHECK_LAUNCH("nmf_camera_rays");
    return NMF_OK;
}

extern "C" int nmf_frame_finish(const float* rgb, const float* depth, const float* normal, const float* acc, float near, float far,
                                const uint8_t* lut, int32_t H, int32_t W, uint8_t* out, void* stream) {
    NMF_REQUIRE(H >= 1 && W >= 1, NMF_EINVAL, "nmf_frame_finish: H or W below 1");
    NMF_REQUIRE(finite_f(near) && finite_f(far), NMF_EINVAL, "nmf_frame_finish: near and far must be finite");
    NMF_REQUIRE(far > near, NMF_EINVAL, "nmf_frame_finish: far must be above near");
    NMF_REQUIRE(rgb || depth || normal || acc, NMF_EINVAL, "nmf_frame_finish: no panel (all four inputs are null)");
    NMF_REQUIRE(out, NMF_EINVAL, "nmf_frame_finish: null out");
    FinishArgs A;
    int n = 0;
    A.o_rgb = rgb ? n++ : -1;
    A.o_depth = depth ? n++ : -1;
    A.o_normal = normal ? n++ : -1;
    A.o_acc = acc ? n++ : -1;
    NMF_REQUIRE((int64_t)H * W * n <= 2147483647LL, NMF_ERANGE, "nmf_frame_finish: more than 2^31 - 1 output pixels");
    A.rgb = rgb; A.depth = depth; A.normal = normal; A.acc = acc;
    A.near = near; A.range = (far - near) + 1e-8f;
    A.lut = lut; A.W = W; A.n_panels = n; A.T = (int64_t)H * W * n; A.out = out;
    const int aligned = ((uintptr_t)out & 3) == 0;
    NMF_LAUNCH(k_frame_finish, dim3((unsigned)cdiv(cdiv(A.T, 4), 256)), dim3(256), 0, (hipStream_t)stream, A, aligned);
    NMF_CHECK_LAUNCH("nmf_frame_finish");
    return NMF_OK;
}
