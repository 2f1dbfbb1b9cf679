// Material maps of the evaluation pass for gfx950 (reference: renderer.py:440-463 writes them, modules/tensor_nerf.py:480-566
// forms them, models/microfacet.py:299-316,572,615-672 defines the per-sample values; nmf_amd/models/microfacet.py Shaded.debug
// restates them on the operator graph).  Per primary ray r with kept samples k:
//   map_X[r] = sum_k w_k X_k + (1 - acc_r) bg
// X = albedo h[0:3] | roughness h[9] | diffuse (1 - Fr) albedo E(n) | tint Fr brdf_rgb | spec, with h = heads(app_k) (heads_eval.hpp),
// E(n) = sum_j conv[j] Y_j(n), Fr = f0 + (1 - f0) clip(1 - |dot(-v, n)|, 0, 1)^5, and spec / brdf_rgb the means of the incoming
// radiance / BRDF weight over the secondary rays of the sample's bounce row (0 for a sample without one).
//
// One lane group per ray (k_segment_sum_group / k_ray_compose_fwd_wave): each lane walks the samples s + lane, s + lane + W, ... and
// evaluates the heads, the irradiance, the Fresnel term and its row's means in registers; the group sums with a fixed shuffle tree.
// The only global writes are the 15 floats of the ray.  W and b of the heads and the 27 SH coefficients sit in LDS (heads.hip:59-62:
// as uniform global addresses they become more scalar loads than the scalar registers hold).
#include <type_traits>

#include "edit_eval.hpp"
#include "heads_eval.hpp"
#include "rows_bwd.hpp"

namespace {

using nmf_heads::F;
using nmf_heads::O;
using nmf_heads::HeadP;

constexpr int NMAP = 15;        // albedo 0-2 | roughness 3-5 | diffuse 6-8 | tint 9-11 | spec 12-14

struct MapsIn {
    const float* app;           // [M][24]
    const float* normals;       // [M][3]
    const float* weight;        // [M]
    const int64_t* offsets;     // [B+1]
    const float* rays;          // [B][6]
    const int32_t* inv;         // [M] bounce row or -1 (NULL: no rows)
    const int64_t* row_off;     // [Mb+1]
    const int32_t* cnt;         // [Mb]
    const float* incoming;      // [R][3]
    const float* brdf;          // [R][3]
    const float* acc;           // [B]
    const float* bg;            // [3]
};

// the material edits of nmf_material_maps_edit: the samples' positions and the table (by value, edit_eval.hpp); NoEdit is what the
// kernel of nmf_material_maps takes in its place (the EDIT = false instantiation has the code it had before edits existed)
struct EditIn {
    const float* xyz;           // [M][xyz_stride]
    int32_t xyz_stride;
    nmf_edit::Table tab;
};
struct NoEdit {
    int32_t unused;
};

template <int W, bool EDIT>
__global__ void __launch_bounds__(256) k_material_maps(MapsIn in, int64_t B, const float* __restrict__ head_W,
                                                       const float* __restrict__ head_b, HeadP hp, const float* __restrict__ conv,
                                                       float* __restrict__ out,
                                                       typename std::conditional<EDIT, EditIn, NoEdit>::type ed) {
#pragma clang fp contract(off)
    __shared__ float s_W[O * F];
    __shared__ float s_b[O];
    __shared__ float s_c[27];
    const int t = threadIdx.x;
    for (int i = t; i < O * F; i += 256) s_W[i] = head_W[i];
    if (t < O) s_b[t] = head_b[t];
    if (t < 27) s_c[t] = conv[t];
    __syncthreads();
    const int64_t r = ((int64_t)blockIdx.x * 256 + t) / W;
    const int lane = t & (W - 1);
    const bool ok = r < B;                       // whole lane groups are in or out; the shuffles below stay inside a group
    const int64_t s = ok ? in.offsets[r] : 0, e = ok ? in.offsets[r + 1] : 0;
    const int64_t rq = ok ? r : 0;
    const float dx = in.rays[rq * 6 + 3], dy = in.rays[rq * 6 + 4], dz = in.rays[rq * 6 + 5];
    float v[13];                                 // albedo 3 | r1 | diffuse 3 | tint 3 | spec 3
#pragma unroll
    for (int q = 0; q < 13; ++q) v[q] = 0.f;
    for (int64_t k = s + lane; k < e; k += W) {
        const float w = in.weight[k];
        if (w == 0.f) continue;                  // contributes nothing to any map
        float f[F], h[O];
        const float4* fq = reinterpret_cast<const float4*>(in.app + k * F);
#pragma unroll
        for (int i = 0; i < F / 4; ++i) {
            const float4 a = fq[i];
            f[4 * i] = a.x; f[4 * i + 1] = a.y; f[4 * i + 2] = a.z; f[4 * i + 3] = a.w;
        }
        // (an opaque zero offset per sample keeps the 275 LDS reads of W and b inside the loop: hoisted out of it they are 275
        // live registers and the kernel runs at one wave per SIMD)
        int z = 0;
        asm volatile("" : "+v"(z));
        nmf_heads::heads_eval(f, s_W + z, s_b + z, hp, h);
        if constexpr (EDIT) {
            const float* __restrict__ p = ed.xyz + k * (int64_t)ed.xyz_stride;
            nmf_edit::edit_apply(h, p[0], p[1], p[2], ed.tab);
        }
        const float nx = in.normals[k * 3], ny = in.normals[k * 3 + 1], nz = in.normals[k * 3 + 2];
        float Y[9];
        nmf_rows::sh9(nx, ny, nz, Y);
        // spec / brdf_rgb: the row's secondary rays, each divided by max(cnt, 1), summed in index order
        float sp[3] = {0.f, 0.f, 0.f}, br[3] = {0.f, 0.f, 0.f};
        const int32_t row = in.inv ? in.inv[k] : -1;
        if (row >= 0) {
            const float ec = (float)max(in.cnt[row], 1);
            for (int64_t j = in.row_off[row]; j < in.row_off[row + 1]; ++j) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sp[c] += in.incoming[j * 3 + c] / ec;
                    br[c] += in.brdf[j * 3 + c] / ec;
                }
            }
        }
        const float cos_t = fabsf((-dx * nx + -dy * ny) + -dz * nz);
        const float x = fminf(fmaxf(1.f - cos_t, 0.f), 1.f);
        const float x5 = powf(x, 5.f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float E = 0.f;
#pragma unroll
            for (int j = 0; j < 9; ++j) E += s_c[j * 3 + c] * Y[j];
            const float f0 = h[6 + c];
            const float Fr = f0 + (1.f - f0) * x5;
            v[c] += w * h[c];
            v[4 + c] += w * ((1.f - Fr) * (h[c] * E));
            v[7 + c] += w * (Fr * br[c]);
            v[10 + c] += w * sp[c];
        }
        v[3] += w * h[9];
    }
#pragma unroll
    for (int q = 0; q < 13; ++q)
        for (int d = W / 2; d > 0; d >>= 1) v[q] += __shfl_down(v[q], d, W);
    if (lane != 0 || !ok) return;
    const float a = 1.f - in.acc[r];
    const float bg[3] = {in.bg[0], in.bg[1], in.bg[2]};
    float* o = out + r * NMAP;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = v[c] + a * bg[c];
        o[3 + c] = v[3] + a * bg[c];
        o[6 + c] = v[4 + c] + a * bg[c];
        o[9 + c] = v[7 + c] + a * bg[c];
        o[12 + c] = v[10 + c] + a * bg[c];
    }
}

template <bool EDIT>
int launch_maps(const char* who, const float* app, const float* normals, const float* weight, const int64_t* offsets, int64_t B, int64_t M,
                const float* rays, const float* head_W, const float* head_b, const HeadP& hp, const float* conv, const int32_t* inv,
                const int64_t* row_off, const int32_t* cnt, int64_t Mb, const float* incoming, const float* brdf, const float* acc,
                const float* bg, float* out, void* stream, const typename std::conditional<EDIT, EditIn, NoEdit>::type& ed) {
    const MapsIn in{app, normals, weight, offsets, rays, Mb > 0 ? inv : nullptr, row_off, cnt, incoming, brdf, acc, bg};
    // lanes per ray from the mean samples per ray: about two samples per lane, whole waves of 64 at most
    const int64_t avg = B > 0 ? M / B : 0;
    hipStream_t st = (hipStream_t)stream;
    if (avg >= 64)
        NMF_LAUNCH_NAMED(EDIT ? "k_material_maps_edit<64>" : "k_material_maps<64>", (k_material_maps<64, EDIT>), dim3((unsigned)cdiv(B, 4)),
                         dim3(256), 0, st, in, B, head_W, head_b, hp, conv, out, ed);
    else if (avg >= 16)
        NMF_LAUNCH_NAMED(EDIT ? "k_material_maps_edit<16>" : "k_material_maps<16>", (k_material_maps<16, EDIT>), dim3((unsigned)cdiv(B, 16)),
                         dim3(256), 0, st, in, B, head_W, head_b, hp, conv, out, ed);
    else
        NMF_LAUNCH_NAMED(EDIT ? "k_material_maps_edit<8>" : "k_material_maps<8>", (k_material_maps<8, EDIT>), dim3((unsigned)cdiv(B, 32)),
                         dim3(256), 0, st, in, B, head_W, head_b, hp, conv, out, ed);
    NMF_CHECK_LAUNCH(who);
    return NMF_OK;
}

}  // namespace

extern "C" int nmf_material_maps(const float* app, const float* normals, const float* weight, const int64_t* offsets, int64_t B,
                                 int64_t M, const float* rays, const float* head_W, const float* head_b, float diffuse_mul,
                                 float diffuse_bias, float tint_bias, float f0_bias, float rough_bias, const float* conv,
                                 const int32_t* inv, const int64_t* row_off, const int32_t* cnt, int64_t Mb, const float* incoming,
                                 const float* brdf_weight, int64_t R, const float* acc, const float* bg, float* out, void* stream) {
    NMF_REQUIRE(B >= 0 && M >= 0 && Mb >= 0 && R >= 0, NMF_EINVAL, "nmf_material_maps: negative size");
    NMF_REQUIRE(Mb <= M && Mb <= R && (Mb > 0 || R == 0), NMF_EINVAL, "nmf_material_maps: need Mb <= M, Mb <= R, R == 0 without rows");
    if (B == 0) return NMF_OK;
    NMF_REQUIRE(offsets && rays && head_W && head_b && conv && acc && bg && out, NMF_EINVAL, "nmf_material_maps: null");
    NMF_REQUIRE(M == 0 || (app && normals && weight), NMF_EINVAL, "nmf_material_maps: null sample input");
    NMF_REQUIRE(Mb == 0 || (inv && row_off && cnt && incoming && brdf_weight), NMF_EINVAL, "nmf_material_maps: null row input");
    const HeadP hp{diffuse_mul, diffuse_bias, tint_bias, f0_bias, rough_bias};
    return launch_maps<false>("nmf_material_maps", app, normals, weight, offsets, B, M, rays, head_W, head_b, hp, conv, inv, row_off, cnt, Mb,
                              incoming, brdf_weight, acc, bg, out, stream, NoEdit{0});
}

extern "C" int nmf_material_maps_edit(const float* app, const float* normals, const float* weight, const int64_t* offsets, int64_t B,
                                      int64_t M, const float* rays, const float* head_W, const float* head_b, float diffuse_mul,
                                      float diffuse_bias, float tint_bias, float f0_bias, float rough_bias, const float* conv,
                                      const int32_t* inv, const int64_t* row_off, const int32_t* cnt, int64_t Mb, const float* incoming,
                                      const float* brdf_weight, int64_t R, const float* acc, const float* bg, float* out,
                                      const float* xyz, int32_t xyz_stride, const float* edits, int32_t n_edits, void* stream) {
    NMF_REQUIRE(B >= 0 && M >= 0 && Mb >= 0 && R >= 0, NMF_EINVAL, "nmf_material_maps_edit: negative size");
    NMF_REQUIRE(Mb <= M && Mb <= R && (Mb > 0 || R == 0), NMF_EINVAL, "nmf_material_maps_edit: need Mb <= M, Mb <= R, R == 0 without rows");
    NMF_REQUIRE(xyz_stride == 3 || xyz_stride == 4, NMF_EINVAL, "nmf_material_maps_edit: xyz_stride must be 3 or 4");
    EditIn ed;
    const int rc = nmf_edit::load_table(edits, n_edits, ed.tab, "nmf_material_maps_edit");
    if (rc != NMF_OK) return rc;
    if (B == 0) return NMF_OK;
    NMF_REQUIRE(offsets && rays && head_W && head_b && conv && acc && bg && out, NMF_EINVAL, "nmf_material_maps_edit: null");
    NMF_REQUIRE(M == 0 || (app && normals && weight), NMF_EINVAL, "nmf_material_maps_edit: null sample input");
    NMF_REQUIRE(Mb == 0 || (inv && row_off && cnt && incoming && brdf_weight), NMF_EINVAL, "nmf_material_maps_edit: null row input");
    NMF_REQUIRE(n_edits == 0 || M == 0 || xyz, NMF_EINVAL, "nmf_material_maps_edit: null positions");
    const HeadP hp{diffuse_mul, diffuse_bias, tint_bias, f0_bias, rough_bias};
    if (n_edits == 0)          // the launch of nmf_material_maps itself
        return launch_maps<false>("nmf_material_maps_edit", app, normals, weight, offsets, B, M, rays, head_W, head_b, hp, conv, inv, row_off,
                                  cnt, Mb, incoming, brdf_weight, acc, bg, out, stream, NoEdit{0});
    ed.xyz = xyz;
    ed.xyz_stride = xyz_stride;
    return launch_maps<true>("nmf_material_maps_edit", app, normals, weight, offsets, B, M, rays, head_W, head_b, hp, conv, inv, row_off, cnt,
                             Mb, incoming, brdf_weight, acc, bg, out, stream, ed);
}
