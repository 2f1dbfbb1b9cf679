// Render-time material edits over stored head rows for gfx950 (include/nmf_hip.h "Material edits"; the semantics are the one
// function nmf_edit::edit_apply of edit_eval.hpp, which k_material_maps of maps.hip applies as well).
//
// One lane per row of 11 floats.  A row is 44 bytes, so no row but every fourth starts on a 16-byte boundary and a lane that
// read its own row from memory would issue 11 dword loads 44 bytes apart (each wave instruction touching 64 rows = 44 cache
// lines' worth of 2816 bytes, 11 times over).  Instead the workgroup moves its tile of 256 rows (2816 consecutive dwords) through
// LDS with coalesced dword accesses in both directions, and a lane picks its row out of LDS at stride 11: odd, so the 64 lanes of
// a ds_read hit 64 different banks.  The edit table arrives by value in the kernel arguments (edit_eval.hpp).
#include "edit_eval.hpp"

namespace {

constexpr int TB = 256;       // rows per workgroup
constexpr int O = 11;

__global__ void __launch_bounds__(TB) k_heads_edit(float* __restrict__ heads, const float* __restrict__ xyz, int32_t xyz_stride,
                                                   int64_t n, nmf_edit::Table tab) {
    __shared__ float s_h[TB * O];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * TB;
    const int rows = (int)((n - row0) < (int64_t)TB ? (n - row0) : (int64_t)TB);      // >= 1: the grid is cdiv(n, TB)
    float* __restrict__ g = heads + row0 * O;
    const int cnt = rows * O;
    for (int i = t; i < cnt; i += TB) s_h[i] = g[i];
    __syncthreads();
    if (t < rows) {
        const float* __restrict__ p = xyz + (row0 + t) * (int64_t)xyz_stride;
        const float x = p[0], y = p[1], z = p[2];
        float h[O];
#pragma unroll
        for (int j = 0; j < O; ++j) h[j] = s_h[t * O + j];
        nmf_edit::edit_apply(h, x, y, z, tab);
#pragma unroll
        for (int j = 0; j < O; ++j) s_h[t * O + j] = h[j];
    }
    __syncthreads();
    for (int i = t; i < cnt; i += TB) g[i] = s_h[i];
}

}  // namespace

extern "C" int nmf_heads_edit(float* heads, const float* xyz, int32_t xyz_stride, int64_t n, const float* edits, int32_t n_edits,
                              void* stream) {
    NMF_REQUIRE(n >= 0, NMF_EINVAL, "nmf_heads_edit: n < 0");
    NMF_REQUIRE(xyz_stride == 3 || xyz_stride == 4, NMF_EINVAL, "nmf_heads_edit: xyz_stride must be 3 or 4");
    nmf_edit::Table tab;
    const int rc = nmf_edit::load_table(edits, n_edits, tab, "nmf_heads_edit");
    if (rc != NMF_OK) return rc;
    NMF_REQUIRE(n <= (int64_t)0x7fffffff * TB, NMF_ERANGE, "nmf_heads_edit: more rows than one grid covers");
    if (n == 0 || n_edits == 0) return NMF_OK;
    NMF_REQUIRE(heads && xyz, NMF_EINVAL, "nmf_heads_edit: null");
    NMF_LAUNCH(k_heads_edit, dim3((unsigned)cdiv(n, TB)), dim3(TB), 0, (hipStream_t)stream, heads, xyz, xyz_stride, n, tab);
    NMF_CHECK_LAUNCH("nmf_heads_edit");
    return NMF_OK;
}
