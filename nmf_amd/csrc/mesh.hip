// Mesh export: indexed marching cubes over a dense fp32 volume (include/nmf_hip.h, "Mesh export").  Two passes around a scan the
// caller runs: k_mc_count classifies every lattice point's cell and counts what it will write, k_mc_emit writes welded vertices
// and faces at the scanned offsets.  Nothing is appended with atomics: the output order is the lattice order, a pure function
// of the volume.  Built with -ffp-contract=off (build.sh): a vertex position has one defined rounding.
#include "common.hpp"
#include "mc_table.hpp"

namespace {

constexpr int MC_BLOCK = 256;
constexpr int MC_MIN_AXIS = 2, MC_MAX_AXIS = 1024;

// device copy of the generated table (4.25 KB, read through the vector L1: only cells the surface crosses index it)
struct McTable {
    uint8_t num_tri[256];
    int8_t e[256][16];
};
constexpr McTable make_table() {
    McTable t{};
    for (int c = 0; c < 256; ++c) {
        t.num_tri[c] = nmf_mc::kNumTri[c];
        for (int k = 0; k < 16; ++k) t.e[c][k] = nmf_mc::kTri[c][k];
    }
    return t;
}
__device__ const McTable d_table = make_table();

struct McDims {
    int32_t gx, gy, gz;
    int64_t n;                                                                  // gx * gy * gz lattice points
};

// owned edges of a case: bit a set = the +a edge from corner 0 changes sign (corner 0 against corners 1, 2, 4)
__device__ __forceinline__ uint32_t owned_mask(uint32_t c) {
    const uint32_t b0 = c & 1u;
    return (b0 ^ ((c >> 1) & 1u)) | ((b0 ^ ((c >> 2) & 1u)) << 1) | ((b0 ^ ((c >> 4) & 1u)) << 2);
}

// the four insideness bits of the lattice points (i..i+1, j..j+1, k): bit dx + 2 dy.  Indices past the volume repeat the last
// point of the axis, so an edge that leaves the volume never changes sign.  NaN > level is false: a NaN is outside.
__device__ __forceinline__ uint32_t plane_bits(const float* __restrict__ vol, const McDims& d, int32_t i, int32_t j, int32_t k,
                                               float level) {
    const int64_t sx = (int64_t)d.gy * d.gz;
    const int64_t i0 = (int64_t)i * sx, i1 = (int64_t)min(i + 1, d.gx - 1) * sx;
    const int64_t j0 = (int64_t)j * d.gz, j1 = (int64_t)min(j + 1, d.gy - 1) * d.gz;
    uint32_t b = vol[i0 + j0 + k] > level ? 1u : 0u;
    b |= vol[i1 + j0 + k] > level ? 2u : 0u;
    b |= vol[i0 + j1 + k] > level ? 4u : 0u;
    b |= vol[i1 + j1 + k] > level ? 8u : 0u;
    return b;
}

// One thread per lattice point n = (i * gy + j) * gz + k, z fastest: a wave reads rows of the volume.  A thread classifies the
// four points of its own z plane and takes the plane above from the next lane (the thread of point k + 1); only the last lane of
// a wave and the last point of a z row read theirs.  Rows are re-read by the threads of (i-1, j), (i, j-1), (i-1, j-1): those
// hits come from the vector L1 / L2, see DESIGN.md section 10.3.
__global__ __launch_bounds__(MC_BLOCK) void k_mc_count(const float* __restrict__ vol, McDims d, float level,
                                                       uint8_t* __restrict__ cases, int32_t* __restrict__ vcount,
                                                       int32_t* __restrict__ tcount) {
    const int64_t n = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    const bool live = n < d.n;
    const int64_t nn = live ? n : d.n - 1;                                      // dead threads keep the wave's shuffle whole
    const int32_t k = (int32_t)(nn % d.gz);
    const int64_t r = nn / d.gz;
    const int32_t j = (int32_t)(r % d.gy), i = (int32_t)(r / d.gy);
    const uint32_t lo = plane_bits(vol, d, i, j, k, level);
    uint32_t hi = (uint32_t)__shfl_down((int)lo, 1, NMF_WAVE);
    if (k + 1 >= d.gz) hi = lo;                                                 // the z edge leaves the volume
    else if (lane_id() == NMF_WAVE - 1 || n + 1 >= d.n) hi = plane_bits(vol, d, i, j, k + 1, level);
    if (!live) return;
    const uint32_t c = lo | (hi << 4);
    const bool cell = i + 1 < d.gx && j + 1 < d.gy && k + 1 < d.gz;             // a whole cell: triangles; otherwise owned edges only
    cases[n] = (uint8_t)c;
    vcount[n] = __popc(owned_mask(c));
    tcount[n] = cell ? (int32_t)d_table.num_tri[c] : 0;
}

// index of the vertex on edge e of the cell at lattice point n: the owner is the point at the edge's lower end, the vertex is
// the owner's base plus the number of its owned crossing edges along smaller axes
__device__ __forceinline__ int32_t edge_vertex(const uint8_t* __restrict__ cases, const int32_t* __restrict__ vscan, const McDims& d,
                                               int64_t n, int e) {
    const int axis = e >> 2, a = e & 1, b = (e >> 1) & 1;
    const int dx = axis == 0 ? 0 : a, dy = axis == 0 ? a : (axis == 1 ? 0 : b), dz = axis == 2 ? 0 : b;
    const int64_t m = n + ((int64_t)dx * d.gy + dy) * d.gz + dz;
    const uint32_t own = owned_mask(cases[m]);
    const int32_t base = m > 0 ? vscan[m - 1] : 0;
    return base + __popc(own & ((1u << axis) - 1u));
}

// vscan / tscan: INCLUSIVE sums of the counts in lattice order (the counts' own buffers after an in-place scan): point n writes
// from scan[n - 1] (0 for n == 0).  Every store is checked against n_verts / n_faces, so buffers that do not belong together
// cannot make it write outside the outputs.
__global__ __launch_bounds__(MC_BLOCK) void k_mc_emit(const float* __restrict__ vol, McDims d, float level,
                                                      const uint8_t* __restrict__ cases, const int32_t* __restrict__ vscan,
                                                      const int32_t* __restrict__ tscan, int64_t n_verts, int64_t n_faces,
                                                      float* __restrict__ verts, int32_t* __restrict__ faces) {
    const int64_t n = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (n >= d.n) return;
    const uint32_t c = cases[n];
    if (c == 0u || c == 255u) return;
    const int32_t k = (int32_t)(n % d.gz);
    const int64_t r = n / d.gz;
    const int32_t j = (int32_t)(r % d.gy), i = (int32_t)(r / d.gy);
    const uint32_t own = owned_mask(c);
    if (own) {
        int64_t v = n > 0 ? vscan[n - 1] : 0;
        const float a = vol[n];
        const int64_t stride[3] = {(int64_t)d.gy * d.gz, (int64_t)d.gz, 1};
        const float p0[3] = {(float)i, (float)j, (float)k};
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (!((own >> ax) & 1u)) continue;
            const float b = vol[n + stride[ax]];
            const float t = fdiv(fsub(level, a), fsub(b, a));
            if (v < n_verts) {
                verts[3 * v + 0] = ax == 0 ? fadd(p0[0], t) : p0[0];
                verts[3 * v + 1] = ax == 1 ? fadd(p0[1], t) : p0[1];
                verts[3 * v + 2] = ax == 2 ? fadd(p0[2], t) : p0[2];
            }
            ++v;
        }
    }
    if (!(i + 1 < d.gx && j + 1 < d.gy && k + 1 < d.gz)) return;
    const int nt = d_table.num_tri[c];
    int64_t f = n > 0 ? tscan[n - 1] : 0;
    for (int t = 0; t < nt; ++t, ++f) {
        if (f >= n_faces) break;
#pragma unroll
        for (int q = 0; q < 3; ++q) faces[3 * f + q] = edge_vertex(cases, vscan, d, n, d_table.e[c][3 * t + q]);
    }
}

int check_dims(int32_t gx, int32_t gy, int32_t gz, const char* what) {
    NMF_REQUIRE(gx >= MC_MIN_AXIS && gy >= MC_MIN_AXIS && gz >= MC_MIN_AXIS && gx <= MC_MAX_AXIS && gy <= MC_MAX_AXIS &&
                    gz <= MC_MAX_AXIS, NMF_ERANGE, what);
    return NMF_OK;
}

}  // namespace

extern "C" int64_t nmf_mc_workspace_bytes(int32_t gx, int32_t gy, int32_t gz) {
    if (gx <= 0 || gy <= 0 || gz <= 0) return 0;
    return 9 * (int64_t)gx * gy * gz;                                           // two int32 counts and one case byte per lattice point
}

extern "C" int nmf_mc_case_triangles(int case_index, int8_t out[16]) {
    NMF_REQUIRE(out, NMF_EINVAL, "nmf_mc_case_triangles: null");
    NMF_REQUIRE(case_index >= 0 && case_index < 256, NMF_ERANGE, "nmf_mc_case_triangles: case index outside 0..255");
    for (int k = 0; k < 16; ++k) out[k] = nmf_mc::kTri[case_index][k];
    return nmf_mc::kNumTri[case_index];
}

extern "C" int nmf_mc_count(const float* vol, int32_t gx, int32_t gy, int32_t gz, float level, uint8_t* cases, int32_t* vcount,
                            int32_t* tcount, void* stream) {
    NMF_REQUIRE(vol && cases && vcount && tcount, NMF_EINVAL, "nmf_mc_count: null pointer");
    if (int rc = check_dims(gx, gy, gz, "nmf_mc_count: every axis must have 2..1024 points")) return rc;
    const McDims d{gx, gy, gz, (int64_t)gx * gy * gz};
    NMF_LAUNCH(k_mc_count, dim3((unsigned)cdiv(d.n, MC_BLOCK)), dim3(MC_BLOCK), 0, (hipStream_t)stream, vol, d, level, cases, vcount,
               tcount);
    NMF_CHECK_LAUNCH("nmf_mc_count");
    return NMF_OK;
}

extern "C" int nmf_mc_emit(const float* vol, int32_t gx, int32_t gy, int32_t gz, float level, const uint8_t* cases,
                           const int32_t* vscan, const int32_t* tscan, int64_t n_verts, int64_t n_faces, float* verts,
                           int32_t* faces, void* stream) {
    NMF_REQUIRE(vol && cases && vscan && tscan, NMF_EINVAL, "nmf_mc_emit: null pointer");
    if (int rc = check_dims(gx, gy, gz, "nmf_mc_emit: every axis must have 2..1024 points")) return rc;
    NMF_REQUIRE(n_verts >= 0 && n_faces >= 0, NMF_EINVAL, "nmf_mc_emit: negative size");
    NMF_REQUIRE(n_verts <= INT32_MAX && n_faces <= INT32_MAX / 3, NMF_ERANGE,
                "nmf_mc_emit: V or 3 F passes 2^31 - 1 (int32 face indices)");
    NMF_REQUIRE((verts || n_verts == 0) && (faces || n_faces == 0), NMF_EINVAL, "nmf_mc_emit: null output");
    if (n_verts == 0 && n_faces == 0) return NMF_OK;
    const McDims d{gx, gy, gz, (int64_t)gx * gy * gz};
    NMF_LAUNCH(k_mc_emit, dim3((unsigned)cdiv(d.n, MC_BLOCK)), dim3(MC_BLOCK), 0, (hipStream_t)stream, vol, d, level, cases, vscan,
               tscan, n_verts, n_faces, verts, faces);
    NMF_CHECK_LAUNCH("nmf_mc_emit");
    return NMF_OK;
}
