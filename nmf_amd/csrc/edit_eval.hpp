// Render-time material edits (include/nmf_hip.h, "Material edits") as ONE piece of code for every kernel that applies them
// (k_heads_edit over stored head rows, k_material_maps right after heads_eval): fp32, one rounding per operation in the order
// written, no fma -- the functions below switch contraction off in their own bodies (the way heads_eval.hpp pins its fmas), so the
// bits do not depend on the flags of the file that includes this (maps.hip is built with contraction on; edit.hip is built with
// -ffp-contract=off as well).  nmf_amd/edit.py apply_reference restates it in numpy.
#pragma once
#include <cmath>

#include "common.hpp"

namespace nmf_edit {

constexpr int ROW = NMF_EDIT_ROW;          // 32 floats per edit
constexpr int MAX_EDITS = NMF_EDIT_MAX;    // 16

// The validated table, passed to the kernels BY VALUE: it sits in the kernel-argument segment, the loop over edits indexes it
// with a uniform counter and every entry is a scalar load (no copy to the device to order against the stream, no buffer to own).
struct Table {
    float e[MAX_EDITS * ROW];
    int32_t n;
};

// host: checks the [n_edits][32] table (host memory) and copies it into `t`.  Nothing is launched before this has passed.
static inline int load_table(const float* edits, int32_t n_edits, Table& t, const char* who) {
    char msg[160];
    if (n_edits < 0) { snprintf(msg, sizeof(msg), "%s: n_edits < 0", who); return nmf_fail(NMF_EINVAL, msg); }
    if (n_edits > MAX_EDITS) { snprintf(msg, sizeof(msg), "%s: more than %d edits", who, MAX_EDITS); return nmf_fail(NMF_ERANGE, msg); }
    if (n_edits > 0 && !edits) { snprintf(msg, sizeof(msg), "%s: null edit table", who); return nmf_fail(NMF_EINVAL, msg); }
    memset(&t, 0, sizeof(t));
    t.n = n_edits;
    for (int32_t k = 0; k < n_edits; ++k) {
        const float* E = edits + (size_t)k * ROW;
        const char* bad = nullptr;
        for (int i = 0; i < ROW && !bad; ++i)
            if (!std::isfinite(E[i])) bad = "an entry is not finite";
        if (!bad && !(E[0] == 0.f || E[0] == 1.f || E[0] == 2.f)) bad = "kind is not 0, 1 or 2";
        if (!bad && !(E[1] == 0.f || E[1] == 1.f || E[1] == 2.f)) bad = "target is not 0, 1 or 2";
        if (!bad && !(E[2] == 0.f || E[2] == 1.f)) bad = "invert is not 0 or 1";
        if (!bad && !(E[3] >= 0.f)) bad = "falloff < 0";
        if (!bad && E[0] != 0.f && !(E[7] > 0.f && E[8] > 0.f && E[9] > 0.f)) bad = "half extents / radii must be > 0";
        if (bad) { snprintf(msg, sizeof(msg), "%s: edit %d: %s", who, (int)k, bad); return nmf_fail(NMF_ERANGE, msg); }
        memcpy(t.e + (size_t)k * ROW, E, sizeof(float) * ROW);
    }
    return NMF_OK;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// m == 0 keeps the bits of v, m == 1 gives t, otherwise v + m (t - v)
__device__ __forceinline__ float blend(float v, float t, float m) {
#pragma clang fp contract(off)
    const float o = v + m * (t - v);
    return m == 0.f ? v : (m == 1.f ? t : o);
}

// h: the 11 head outputs of a sample at world position (x, y, z); the edits of `tab` in list order, each on the result of the one
// before.  The loop is not unrolled and `k` is uniform: a handful of scalar loads per edit, whatever the number of edits
// (heads.hip:59 records what hundreds of hoisted uniform loads cost).  h is only ever indexed by constants (no scratch): the
// target picks the three registers with selects.
__device__ __forceinline__ void edit_apply(float (&h)[11], float x, float y, float z, const Table& tab) {
#pragma clang fp contract(off)
    const int K = tab.n;
#pragma clang loop unroll(disable)
    for (int k = 0; k < K; ++k) {
        const float* __restrict__ E = tab.e + k * ROW;
        const float kind = E[0], target = E[1], invert = E[2], falloff = E[3];
        float m = 1.f;
        if (kind != 0.f) {
            const float px = x - E[4], py = y - E[5], pz = z - E[6];
            const float hx = E[7], hy = E[8], hz = E[9];
            float d;
            if (kind == 1.f) {
                d = fmaxf(fmaxf(fabsf(px) - hx, fabsf(py) - hy), fabsf(pz) - hz);
            } else {
                const float q0 = px / hx, q1 = py / hy, q2 = pz / hz;
                const float r = sqrtf((q0 * q0 + q1 * q1) + q2 * q2);
                d = (r - 1.f) * fminf(fminf(hx, hy), hz);
            }
            if (falloff == 0.f) {
                m = d <= 0.f ? 1.f : 0.f;
            } else {
                const float s = clamp01(1.f - d / falloff);
                m = (s * s) * (3.f - 2.f * s);
            }
        }
        if (invert != 0.f) m = 1.f - m;
        if (target == 2.f) {
            const float a = E[10], b = E[19];
#pragma unroll
            for (int j = 9; j < 11; ++j) {
                const float t = fminf(fmaxf(a * h[j] + b, 1e-2f), 1.f);
                h[j] = blend(h[j], t, m);
            }
        } else {
            const bool alb = target == 0.f;
            const float v0 = alb ? h[0] : h[6], v1 = alb ? h[1] : h[7], v2 = alb ? h[2] : h[8];
            float o[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float t = ((E[10 + 3 * c] * v0 + E[11 + 3 * c] * v1) + E[12 + 3 * c] * v2) + E[19 + c];
                o[c] = blend(c == 0 ? v0 : (c == 1 ? v1 : v2), clamp01(t), m);
            }
            if (alb) { h[0] = o[0]; h[1] = o[1]; h[2] = o[2]; }
            else { h[6] = o[0]; h[7] = o[1]; h[8] = o[2]; }
        }
    }
}

}  // namespace nmf_edit
