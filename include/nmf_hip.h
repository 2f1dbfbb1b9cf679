/*
 * nmf_hip.h -- C ABI of libnmf_hip.so, the MI355X (gfx950) kernels beneath the
 * microfacet_tensorf2 render/train hot path of half-potato/nmf.
 *
 * The reference has no FFI on this path (it is pure PyTorch); every entry point
 * below replaces a span of reference Python that the host-side mirror classes in nmf_amd/ call
 * instead (file:line of the reference given per function, relative to /root/reference).
 *
 * Conventions
 *   - extern "C", plain pointers, int64_t sizes, hipStream_t passed as void*.
 *   - The CALLER allocates every output (and zeroes the ones documented as "accumulated").
 *   - The library never allocates persistent memory, never frees and never synchronises the
 *     stream; one call = a fixed small number of kernel launches on the given stream.
 *   - Return value: 0 = ok, negative = bad argument (NMF_E*), positive = hipError_t.
 *     nmf_last_error_string() describes the last failure on the calling thread.
 *   - All device pointers must be valid on the current device (hipSetDevice by the caller).
 *   - fp32 throughout; tables are CHANNEL-LAST: plane [G_h][G_w][C], line [G][C]
 *     (= torch.channels_last storage of the reference's [1,C,G,G] / [1,C,G,1] parameters).
 */
#ifndef NMF_HIP_H
#define NMF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NMF_OK 0
#define NMF_EINVAL (-1)   /* null pointer / bad size */
#define NMF_ERANGE (-2)   /* size outside compiled limits (channels, steps ...) */

#define NMF_DENSITY_C 16  /* density_n_comp, configs/field/tensorf_og.yaml */
#define NMF_APP_C 24      /* appearance_n_comp */
#define NMF_APP_DIM 24    /* app_dim (basis_mat rows) */
#define NMF_MLP_IN 66     /* MLPBRDF input width, modules/brdf.py:73-120 */
#define NMF_MLP_HID 64

/* Bumped with every incompatible change of a prototype or of a workspace size.  nmf_version() returns the value the LIBRARY
 * was built with; a separately built caller (nmf_amd/lib/_nmf_host.so) compares it with the value it was compiled against. */
#define NMF_ABI_VERSION 125
int nmf_version(void);
const char* nmf_last_error_string(void);

/* Runtime plumbing for host-side drivers that are built without the HIP headers (nmf_amd/csrc/host_ext.cpp is plain g++ against
 * the torch headers): events without timing, stream ordering and the start of a size read-back into pinned host memory.  The
 * reference has no counterpart (its sizes come back through tensor.item() / .sum() host syncs, e.g. samplers/alphagrid.py:357).
 * nmf_event_synchronize is the one BLOCKING entry point of the library. */
int nmf_event_create(void** event);
int nmf_event_create_timed(void** event);                        /* with timestamps, for nmf_event_elapsed_ms */
int nmf_event_elapsed_ms(void* start, void* stop, float* ms);   /* both recorded and complete */
int nmf_event_destroy(void* event);
int nmf_event_record(void* event, void* stream);
int nmf_event_synchronize(void* event);
/* Size read-back without a copy command or an event (runtime plumbing like the calls above; the reference reads its sizes with
 * implicit .item() synchronisations, e.g. samplers/alphagrid.py:353-364, models/microfacet.py:318-331): the sizes are published by a
 * one-thread kernel into mapped, coherent host memory [value0, value1, seq] and the host spins on seq.  nmf_wait_seq is blocking. */
int nmf_host_alloc_mapped(void** host_ptr, void** dev_ptr, int64_t nbytes);
int nmf_host_free_mapped(void* host_ptr);
int nmf_publish_i64x2(const int64_t* src_dev, void* dst_mapped_dev, int64_t seq, void* stream);
int nmf_wait_seq(const void* host_ptr, int64_t seq, double timeout_s);
int nmf_stream_wait_event(void* stream, void* event);
/* Launch probe (measurement plumbing: bench.py's per-kernel HIP-event timing on the launching stream): when set, EVERY kernel launch
 * of the library calls probe(kernel_name, stream, 0) in front of and probe(kernel_name, stream, 1) behind the launch, on the calling
 * thread.  kernel_name is the kernel's identifier as rocprofv3 --kernel-trace prints it (without arguments).  NULL removes it. */
typedef void (*nmf_launch_probe_fn)(const char* kernel_name, void* stream, int phase);
int nmf_set_launch_probe(void (*probe)(const char* kernel_name, void* stream, int phase));

/* ------------------------------------------------------------------------------------------
 * Sampler: AlphaGridSampler.sample / sample_ray / AlphaGridMask.sample_alpha
 * (samplers/alphagrid.py:131-207, 23-45, 279-370).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    float aabb_min[3], aabb_max[3];
    float alpha_inv[3];   /* AlphaGridMask.invgrid_size = 1/aabbSize*2 (alphagrid.py:12)          */
    float stepsize;       /* rf.stepsize (fp32)                                                   */
    float half_step;      /* stepsize / 2 as torch computes it (alphagrid.py:171)                 */
    float near_t, far_t;  /* near_far, near replaced by override_near for secondary rays          */
    float focal;          /* 4th coordinate = t / focal (alphagrid.py:200)                        */
    int32_t n_steps;      /* N = nSamples (<= 4096)                                               */
    int32_t grid[3];      /* alpha volume size (x,y,z); 0 => no alpha mask                        */
    int32_t is_train;     /* 1: cumulative jitter (alphagrid.py:168-173); 0: stepsize*k (:190)    */
    uint64_t seed;        /* Philox seed used when jitter == NULL and is_train                    */
    uint64_t offset;      /* Philox stream offset (advance per call)                              */
    float occ_min[3], occ_max[3];  /* optional world-space box around every point whose 8-corner footprint can touch a
                                    * set alpha bit (tight box of the set voxels grown by one voxel + margin): the
                                    * marcher stops a ray once it has left this box (nothing can be kept beyond it).
                                    * occ_min > occ_max on any axis = not provided.  Results are unchanged.          */
} nmf_march_params;

/* float 0/1 volume [gz][gy][gx] -> bitfield, bit i of word i/32 = volume[i] > 0
 * (the ">0 after trilinear sampling" test of alphagrid.py:341-346 only needs occupancy bits). */
int nmf_alpha_pack(const float* volume, int64_t n_voxels, uint32_t* bits, void* stream);

/* Pass 1: per-ray validity bitmask ([B][W] uint64, W = ceil(N/64), bit k = step k kept) and
 * per-ray kept count.  jitter: [B][N] uniforms in [0,1) or NULL (Philox). */
int nmf_march_count(const nmf_march_params* p, const float* rays /*[B][6]*/, int64_t B,
                    const float* jitter, const uint32_t* alpha_bits, const uint32_t* alpha_coarse,
                    uint64_t* valid_bits, int32_t* counts, void* stream);
/* Optional accelerator of the occupancy test: one bit per 8^3-voxel cell = OR of the 9^3 fine bits any point of the
 * cell can touch (nmf_alpha_coarse_words(grid) uint32 words).  nmf_march_count stages it in LDS and skips the 8-corner
 * test where it is clear; results are unchanged.  alpha_coarse may be NULL. */
int nmf_alpha_coarse(const uint32_t* alpha_bits, const int32_t grid[3], uint32_t* coarse, void* stream);
int64_t nmf_alpha_coarse_words(const int32_t grid[3]);

/* Pass 2: exclusive scan of counts + the sample budget of alphagrid.py:353-364:
 * if max_samples > 0 and sum(counts) > max_samples then whole_valid[i] = cumsum(counts)[i] < max_samples
 * else all rays valid.  totals[0] = M (kept samples of valid rays), totals[1] = b (valid rays; they
 * are always a prefix).  offsets has B+1 entries (entries past b are clamped to M).
 * publish_mapped_dev (nmf_host_alloc_mapped's device pointer, or NULL): the thread that writes totals also PUBLISHES them,
 * [M, b, publish_seq], into mapped host memory for a host that waits with nmf_wait_seq -- the size read-back of
 * alphagrid.py:353-364 (`ray_valid.sum() > max_samples`, a host sync) without a launch of its own. */
int nmf_march_scan(const int32_t* counts, int64_t B, int64_t max_samples, int64_t* offsets,
                   uint8_t* whole_valid, int64_t* totals, void* workspace, int64_t workspace_bytes,
                   void* publish_mapped_dev, int64_t publish_seq, void* stream);
int64_t nmf_march_scan_workspace_bytes(int64_t B);

/* Pass 3: emit the compacted samples of the first b rays: xyzt [M][4] (world xyz, t/focal),
 * ray_id [M], step_id [M], z [M], dist [M] (= z[k+1]-z[k] over ALL candidates, 0 for the last,
 * alphagrid.py:348-350).  Any output pointer may be NULL. */
int nmf_march_fill(const nmf_march_params* p, const float* rays, int64_t b, const float* jitter,
                   const uint64_t* valid_bits, const int64_t* offsets, float* xyzt, int32_t* ray_id,
                   int32_t* step_id, float* z, float* dist, void* stream);

/* Dense views for API compatibility / parity tests: ray_valid [b][N] bool and z_vals [b][N]. */
int nmf_march_dense(const nmf_march_params* p, const float* rays, int64_t b, const float* jitter,
                    const uint64_t* valid_bits, uint8_t* ray_valid, float* z_vals, void* stream);

/* ------------------------------------------------------------------------------------------
 * TensoRF VM field: TensorVMSplit._compute_densityfeature / _compute_appfeature /
 * TensorBase.compute_normals (fields/tensoRF.py:181-205,392-405; fields/tensor_base.py:66-129)
 * with the derivative stencil of GridSampler2D.backward (modules/grid_sample_Cinf.py:109-325).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    float aabb_min[3];
    float inv_size[3];     /* rf.invaabbSize = 2/aabbSize (tensor_base.py:58)                     */
    float density_shift;   /* tensor_base.py:85                                                    */
    int32_t grid;          /* G (cubic)                                                            */
    float stencil[5];      /* centre row of the 5x5 x-stencil; rows above/below via stencil_off   */
    float stencil_off[5];  /* rows i=1 and i=3 of the x-stencil (grid_sample_Cinf.py:218-233)     */
} nmf_vm_params;

/* Derived density tables, rebuilt whenever the density factors change:
 * dpk[i] [G][G][48] = (P | conv_x(P) | conv_y(P)) per texel, dlk[i] [G][32] = (L | conv(L)). */
int nmf_vm_pack_density(const nmf_vm_params* p, const float* const planes[3],
                        const float* const lines[3], float* const dpk[3], float* const dlk[3],
                        void* stream);

/* Forward query of M_cap world-space samples.  Outputs (any may be NULL):
 * sigma_feat [M], sigma [M] (softplus(clamp(f,-15,1e3)+shift)), grad [M][3] (d sigma_feat/d xyz,
 * reference units), normal [M][3] = normalize(-grad), app [M][24], coef [M][72] (plane*line
 * products, saved for the basis_mat gradient).  Density outputs need dpk/dlk, appearance outputs
 * need app_planes/app_lines/basis ([24][72] row-major).
 * tables_bf16 (BASELINE configs[1], train.py:540 `fp16` autocast is the reference's only precision hook): 0 = every factor
 * table is fp32; != 0 = every table is stored as bfloat16 (the upper 16 bits of the fp32 pattern) -- half the bytes per tap --
 * with fp32 arithmetic.  The caller keeps fp32 master tables (Adam, backward walk) and refreshes the bf16 copies after each
 * optimizer step (nmf_multi_copy with dst_is_f64 = 2).
 * M_live (DEVICE, may be NULL): the live sample count when it is still on the device (e.g. totals[0] of nmf_march_scan): the
 * launch is sized by the bound M_cap the caller allocated for (sampler.max_samples, samplers/alphagrid.py:353-364), samples at
 * or beyond *M_live are neither read nor written.  Lets a caller queue the level-0 pipeline behind the scan without waiting
 * for its sizes.  Only the general query (density with grad or normal) takes it. */
int nmf_vm_query_fwd(const nmf_vm_params* p, const float* xyzt, int64_t M_cap, const int64_t* M_live,
                     const void* const dpk[3], const void* const dlk[3], const void* const app_planes[3],
                     const void* const app_lines[3], int32_t tables_bf16, const float* basis, float* sigma_feat,
                     float* sigma, float* grad, float* normal, float* app, float* coef, void* stream);
/* Density VALUE of M samples from the density factors THEMSELVES: planes[i] [G][G][16] (channel-last storage of
 * rf.density_rf.app_plane.i), lines[i] [G][16] -- what fields/tensoRF.py:181-190 + tensor_base.py:85 compute, for the levels
 * of a pass that need no normals (nmf_amd/fast_step.py "sparse normals").  Same taps, same order of the sums as
 * nmf_vm_query_fwd: identical bits; it touches a third of the cache lines the packed value + derivative tables spread the same
 * numbers over.  tables_bf16 != 0: bfloat16 copies of the factors. */
int nmf_vm_query_sigma(const nmf_vm_params* p, const float* xyzt, int64_t M, const void* const planes[3],
                       const void* const lines[3], int32_t tables_bf16, float* sigma_feat, float* sigma, void* stream);
/* The density part of the query (value, sigma, gradient, normal; any output may be NULL) for a FEW rows -- the bounce rows
 * of a re-traced level, where the training pass needs normals (fields/tensor_base.py:66-129 on xyz[bounce_mask]) -- with
 * 16 lanes per row (one per plane tap); the sums are combined in nmf_vm_query_fwd's order: identical bits.
 * dpk / dlk: the packed tables of nmf_vm_pack_density, fp32 or (tables_bf16 != 0) bfloat16. */
int nmf_vm_query_rows(const nmf_vm_params* p, const float* xyzt, int64_t M, const void* const dpk[3],
                      const void* const dlk[3], int32_t tables_bf16, float* sigma_feat, float* sigma, float* grad,
                      float* normal, void* stream);

/* Backward over the concatenation of up to NMF_VM_MAX_SEGMENTS sample sets (no copy): one training pass queries the field for
 * the primary and for the re-traced rays (tensor_nerf.py:286-393 at recur 0 and 1); their adjoints all land in the same
 * tables, so walking them together bins once and flushes every brick both sets touch once.
 * Per set: upstream adjoints (any may be NULL) d_sigma [M] (wrt activated sigma), d_sigma_feat [M] (wrt the raw feature,
 * added to the former's contribution), d_normal [M][3], d_app [M][24]; sigma_feat / grad are the saved forward outputs.  All
 * non-empty segments must provide the same set of adjoints (d_sigma / d_normal / d_app NULL-ness).
 * Accumulates into g_dpk[i] [G][G][48], g_dlk[i] [G][32], g_app_planes[i] [G][G][24], g_app_lines[i] [G][24],
 * g_basis [24][72] (basis_mat, may be NULL) -- caller zeroes them.
 * Samples are counting-sorted by 8^3-voxel brick and reduced in LDS per brick (see vm.hip).
 * workspace: nmf_vm_bwd_workspace_bytes(total M, grid) bytes of scratch (brick ids, records in brick order, and -- without
 * `clean` -- the bin counters); contents are undefined on return.
 * clean (may be NULL: the counters are then zeroed by memset launches of this call), for a caller that walks again and again
 * (a training loop: train.py:497-747 calls backward() every iteration): the counters of the brick sort, the chunk words of its
 * scan and the scratch copies of the basis_mat gradient live in `clean`, nmf_vm_bwd_clean_bytes(grid) bytes of device memory
 * (16-byte aligned) that are ZERO on entry -- zeroed once, when allocated -- and zero again when the kernels of the call have
 * run (each clears what it has consumed).  No memset launch per walk (two for an appearance walk: 3.5 us + a launch gap each on
 * the serial tail of a step).  One scratch per walk that may be in flight. */
#define NMF_VM_MAX_SEGMENTS 4
typedef struct nmf_vm_bwd_segment {
    const float* xyzt;          /* [M][4] */
    int64_t M;
    const float* sigma_feat;    /* [M]    saved forward outputs */
    const float* grad;          /* [M][3] */
    const float* d_sigma;       /* [M]    upstream adjoints, any may be NULL */
    const float* d_sigma_feat;  /* [M] */
    const float* d_normal;      /* [M][3] */
    const float* d_app;         /* [M][24] */
} nmf_vm_bwd_segment;
int nmf_vm_query_bwd_segments(const nmf_vm_params* p, const nmf_vm_bwd_segment* segs /*HOST array*/, int32_t n_segs,
                              const float* const dpk[3], const float* const dlk[3],
                              const float* const app_planes[3], const float* const app_lines[3],
                              const float* basis, float* const g_dpk[3], float* const g_dlk[3],
                              float* const g_app_planes[3], float* const g_app_lines[3], float* g_basis,
                              void* clean, int64_t clean_bytes, void* workspace, int64_t workspace_bytes, void* stream);
int64_t nmf_vm_bwd_workspace_bytes(int64_t M, int32_t grid);
int64_t nmf_vm_bwd_clean_bytes(int32_t grid);

/* Folds the packed gradient back onto the factors (transpose of nmf_vm_pack_density):
 * g_planes[i] [G][G][16], g_lines[i] [G][16] are OVERWRITTEN.
 * x_planes / x_lines / l1_scale_dev (all NULL or all set): the gradient of the density L1 term is added in the same pass,
 * g += l1_scale_dev[0] * sgn(x) / numel(x) for each of the six density parameters x (fields/tensoRF.py:332-340 `density_L1`,
 * weighted by train.py:640-677), given in the storage order of the gradients.  Same bits as the plain unpack followed by
 * nmf_l1_mean_bwd(accumulate), one launch less at the end of a step. */
int nmf_vm_unpack_density_grad(const nmf_vm_params* p, const float* const g_dpk[3], const float* const g_dlk[3],
                               float* const g_planes[3], float* const g_lines[3], const float* const x_planes[3],
                               const float* const x_lines[3], const float* l1_scale_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Compositing: raw2alpha (modules/tensor_nerf.py:19-35) and row_mask_sum
 * (modules/row_mask_sum.py:15-22), segmented by the ray offsets of nmf_march_scan.
 * ---------------------------------------------------------------------------------------- */
int nmf_composite_fwd(const float* sigma, const float* dist, const int64_t* offsets, int64_t b,
                      float distance_scale, float* weight /*[M]*/, float* acc /*[b]*/, void* stream);
int nmf_composite_bwd(const float* sigma, const float* dist, const float* weight,
                      const int64_t* offsets, int64_t b, float distance_scale,
                      const float* d_weight /*[M]*/, float* d_sigma /*[M]*/, void* stream);
/* out[r][d] = sum_{k in segment r} (scale ? scale[k] : 1) * vals[k][d], D = 1..4.  lanes = 1: one lane per segment,
 * added in index order (fp32, reproduces scatter_add_ on the CPU bit for bit); lanes = 8: eight lanes per segment and a
 * shuffle tree (different fp32 rounding; for the adjoint reductions over the secondary rays of a bounce point). */
int nmf_segment_sum(const float* vals, const float* scale, const int64_t* offsets, int64_t n_seg,
                    int32_t D, int32_t lanes, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Environment map: IntegralEquirect (modules/integral_equirect.py:18-173,373-504), activation 'exp'.
 * bg_mat / activated / sat are [3][H][W] fp32.  The summed-area table reproduces torch's CPU
 * rounding (float64 running sums rounded per element, H then W, :433).
 * scalars_dev (optional, DEVICE float[3] = mipbias, brightness, mul) overrides the by-value scalars so that the
 * three learnable 0-d parameters never have to be read back to the host.
 * ---------------------------------------------------------------------------------------- */
/* activated = exp(min(brightness + mul*bg_mat, 20)); sat = cumsum_W(cumsum_H(activated/1000));
 * pole_rows [2][3] (optional) = mean of the first / last row of `activated` per channel (:499-502).
 * sat_i4 [H][W][4] (optional) = the same table with the channels interleaved (4th lane unwritten): the lookups read one
 * 16-byte texel per tap from it instead of three 4-byte values on three planes (layout = 1 below). */
int nmf_sat_build(const float* bg_mat, int32_t H, int32_t W, float brightness, float mul,
                  const float* scalars_dev, float* activated, float* sat, float* pole_rows, float* sat_i4, void* stream);
/* SH projection of prefiltered lookups (modules/integral_equirect.py:324-360, no gradient): coeffs[k][c] =
 * sum_i wq[i][k] * vals[i][c] over n lattice directions (vals [n][3] from nmf_sat_lookup_fwd, wq [n][K] = quadrature
 * weight x SH basis), conv[k][c] = sh_A[k] * coeffs[k][c] / pi (conv / sh_A may be NULL). */
int nmf_sh_project(const float* vals, const float* wq, int64_t n, int32_t K, const float* sh_A, float* coeffs,
                   float* conv, void* stream);
/* d_sat = channel-interleaved adjoint table [H][W][4] (4th lane unused; accumulated by nmf_sat_lookup_bwd;
 * DESTROYED here) -> d_bg [3][H][W] (overwritten).
 * d_pole [2][3]: adjoint of the (top,bottom) pole-row means, may be NULL. */
int nmf_sat_build_bwd(float* d_sat, const float* bg_mat, const float* activated, int32_t H, int32_t W,
                      float brightness, float mul, const float* scalars_dev, const float* d_pole, float* d_bg,
                      void* stream);
/* out[r] = prefiltered radiance along dirs[r] for log-solid-angle sa[r] (IntegralEquirect.forward).
 * pole_rows [2][3] = mean of the first / last row of `activated` (:499-502).
 * dirs_ld = row pitch of dirs in floats: 3 for [R][3] directions, 6 for [R][6] ray rows (origin | direction) whose
 * direction is columns 3..5 -- secondary rays are looked up without slicing them (tensor_nerf.py:302-317).
 * layout: 0 = sat is the planar table [3][H][W], 1 = sat is nmf_sat_build's interleaved sat_i4 [H][W][4]; the results
 * are bit-identical. */
int nmf_sat_lookup_fwd(const float* sat, int32_t H, int32_t W, const float* dirs, int32_t dirs_ld,
                       const float* sa /*[R]*/, int64_t R, float mipbias, const float* scalars_dev,
                       const float* pole_rows, int32_t layout, float* out /*[R][3]*/, void* stream);
/* Adjoints: d_sat [H][W][4] (channel-interleaved so that 8 lanes share one 32-byte atomic run, see csrc/env.hip) and
 * d_pole [2][3] are ACCUMULATED (caller zeroes), d_dirs [R][dirs_ld] is overwritten (with dirs_ld = 6 the origin
 * columns are written as zeros), d_mipbias [1] accumulated.  d_sat / d_dirs / d_mipbias may be NULL. */
int nmf_sat_lookup_bwd(const float* sat, int32_t H, int32_t W, const float* dirs, int32_t dirs_ld, const float* sa,
                       int64_t R, float mipbias, const float* scalars_dev, int32_t layout, const float* d_out /*[R][3]*/,
                       float* d_sat, float* d_pole, float* d_dirs, float* d_mipbias, void* stream);
/* The same adjoints for LARGE lookup counts (autograd of modules/integral_equirect.py:18-173,409-504): the table adjoint is
 * binned instead of scattered with float atomics -- corners counted per 32 x 64-texel SAT tile, written as records into the
 * caller's workspace, accumulated per tile in LDS as 64-bit fixed point (integer LDS atomics run ~8x faster than float
 * atomics on gfx950, and the sums do not depend on the order) and flushed once.  d_sat must be given.  workspace: 16-byte
 * aligned device memory of nmf_sat_lookup_bwd_workspace_bytes(R) bytes (content irrelevant, overwritten): a header, one
 * 32-bit slot per (workgroup of 256 lookups, tile) -- the counting pass hands every workgroup its place in each tile's range,
 * so the record pass walks the footprints once -- and the record pool.  A smaller pool still gives correct results (corners
 * that do not fit take the float atomics); a workspace without room for header + slots + one record is NMF_EINVAL.  Four
 * launches on `stream`. */
int64_t nmf_sat_lookup_bwd_workspace_bytes(int64_t R);
int nmf_sat_lookup_bwd_binned(const float* sat, int32_t H, int32_t W, const float* dirs, int32_t dirs_ld, const float* sa,
                              int64_t R, float mipbias, const float* scalars_dev, int32_t layout,
                              const float* d_out /*[R][3]*/, float* d_sat, float* d_pole, float* d_dirs, float* d_mipbias,
                              void* workspace, int64_t workspace_bytes, void* stream);
/* The two halves of that adjoint as calls of their own, for a caller whose dependency chain needs d_dirs only (the backward of the
 * bounce rays: the sampler's adjoint waits for d_dirs, nothing before the end of the step for d_sat):
 *   nmf_sat_lookup_bwd_dirs                       d_dirs, d_mipbias (both optional), d_pole -- the forward on dual numbers, one launch
 *   nmf_sat_lookup_bwd_binned with d_pole = NULL  d_sat alone (d_dirs, d_mipbias must be NULL too): the three passes without the
 *                                                 dual-number workgroups riding in them, on any other stream
 * Together they add exactly what one full call adds (the table role never touches the pole rows). */
int nmf_sat_lookup_bwd_dirs(const float* sat, int32_t H, int32_t W, const float* dirs, int32_t dirs_ld, const float* sa,
                            int64_t R, float mipbias, const float* scalars_dev, int32_t layout, const float* d_out /*[R][3]*/,
                            float* d_pole, float* d_dirs, float* d_mipbias, void* stream);

/* ------------------------------------------------------------------------------------------
 * Shading helpers.
 * ---------------------------------------------------------------------------------------- */
/* select_bounces (modules/pt_selectors.py:5-60): counts[i] = clamp(floor(pt_i), 0, 400) with
 *   mode 0 (recursion 0): pt = w*mul + u - 0.5                       (mul = rays_per_ray)
 *   mode 1 (recursion>=1): pt = (w + 1e-3*u) / sum_w * mul + add     (sum_w = clip(sum(w + 1e-3 u), 1e-3))
 * sum_w_dev (optional DEVICE scalar) overrides sum_w, so the host need not read the sum back.
 * The dense ray_mask of the reference is the per-row prefix [0, counts[i]). */
int nmf_select_bounces(const float* weights, const float* u, int64_t M, int32_t mode, float mul,
                       float add, float sum_w, const float* sum_w_dev, int32_t* counts, void* stream);
/* Normaliser of the level >= 1 selection above (pt_selectors.py:24-31), on the device in one launch:
 * total = clip(float(sum(weights) + 1e-3 * (sum(u) + extra)), 1e-3), float64 sums.  `extra` = the caller's value for the sum
 * of the uniforms at the culled entries of the dense matrix.  workspace: NMF_SELECT_TOTAL_WS doubles the caller zeroes ONCE
 * (a ticket + per-workgroup partial sums that the last workgroup adds in workgroup order: the result does not depend on the
 * scheduling; the kernel leaves the ticket zeroed); one workspace per stream.  The result is what nmf_select_bounces takes as
 * sum_w_dev. */
#define NMF_SELECT_TOTAL_WS 258
int nmf_select_total(const float* weights, const float* u, int64_t M, double extra, double* workspace, float* total,
                     void* stream);
/* Adjoint of the bounce rows' view vector (V = -ray direction: bV = -viewdirs, models/microfacet.py:354) scattered to the
 * rays: d_rays[ray_id[bidx[row]]][3..5] -= dv_a[row] (+ dv_b[row]); dv_* rows of pitch lda / ldb floats, dv_b nullable. */
int nmf_view_adjoint_to_rays(const int32_t* ray_id, const int32_t* bidx, const float* dv_a, int32_t lda, const float* dv_b,
                             int32_t ldb, int64_t Mb, float* d_rays, void* stream);
/* seg_id[r] / local[r] for r in [offsets[i], offsets[i+1]) = i / r - offsets[i]  (= torch.where(ray_mask)). */
int nmf_expand_segments(const int64_t* offsets, int64_t n_seg, int32_t* seg_id, int32_t* local,
                        void* stream);
/* Secondary rays of the compact ray list (ray i belongs to bounce row row_of_ray[i], is its j_of_ray[i]-th ray):
 * PseudoRandomSampler.draw + GGXSampler.sample/compute_prob + the per-ray glue of Microfacet.forward
 * (brdf_samplers/base.py:11-20, brdf_samplers/ggx.py:61-268, models/microfacet.py:377-456).
 * Rows: V (to viewer), N (flipped to the viewer), r (roughness), x (bounce point), off [Mb][2] (uniform draws, the
 * 0.25 scale is applied inside), cnt (rays per row); sobol [1024][2].  Outputs per ray: L [R][3], half/diff vectors in
 * the local frame [R][3], lpdf [R], mipval [R] = -log(cnt) - lpdf, rays [R][6] = (x + 5e-3 L, L). */
int nmf_ggx_rays_fwd(const float* V_rows, const float* N_rows, const float* r_rows, const float* x_rows,
                     const float* off_rows, const int32_t* cnt_rows, const float* sobol,
                     const int32_t* row_of_ray, const int32_t* j_of_ray, int64_t R, float* L,
                     float* half_local, float* diff_local, float* lpdf, float* mipval, float* rays, void* stream);
/* GGXSampler.compute_prob (brdf_samplers/ggx.py:228-268, isotropic r2 = r1): pdf of a sampled direction from the
 * local-frame incoming / outgoing / half vectors [R][3] and the roughness [R]; 0 below the horizon (dir_in.z <= 0). */
int nmf_ggx_prob(const float* dir_in_local, const float* dir_out_local, const float* half_local, const float* rough,
                 int64_t R, float* prob, void* stream);
/* d_nr [R][4] = (dL/dN)^T g | (dL/dr)^T g per ray (dual-number evaluation of the same sampler); reduce per row.
 * g = dL + d_rays[:,3:6] + 5e-3 d_rays[:,0:3]  (adjoints of L [R][3] and of the bounce rays [R][6]; either may be NULL). */
int nmf_ggx_rays_bwd(const float* V_rows, const float* N_rows, const float* r_rows, const float* off_rows,
                     const float* sobol, const int32_t* row_of_ray, const int32_t* j_of_ray, int64_t R,
                     const float* dL, const float* d_rays, float* d_nr, void* stream);
/* Same with the view direction as a third differentiable input: d_nrv [R][7] = (dN | dr | dV).  The rays of recursion
 * level >= 1 look along the direction the level above sampled (viewdirs = rays[:, 3:6], modules/tensor_nerf.py:262, is part
 * of the graph: bV = -viewdirs, models/microfacet.py:354), so their radiance back-propagates into that direction. */
int nmf_ggx_rays_bwd_view(const float* V_rows, const float* N_rows, const float* r_rows, const float* off_rows,
                          const float* sobol, const int32_t* row_of_ray, const int32_t* j_of_ray, int64_t R,
                          const float* dL, const float* d_rays, float* d_nrv, void* stream);
/* Fresnel-Schlick mix (models/microfacet.py:595-613): contrib [R][3] = (F Li brdf + (1-F) diffuse) / cnt with
 * F = f0 + (1-f0)(1-|V.H|)^5, H = normalize((V+L)/2); sum contrib per row for reflect_rgb. */
int nmf_shade_mix_fwd(const float* V_rows, const float* f0_rows, const float* diffuse_rows,
                      const int32_t* cnt_rows, const int32_t* row_of_ray, int64_t R, const float* L,
                      const float* incoming, const float* brdf, float* contrib, void* stream);
/* d_rows [Mb][3] = adjoint of the row sums.  d_incoming, d_brdf, dL [R][3] overwritten;
 * d_f0diff [R][6] = per-ray (d f0 | d diffuse), reduce per row. */
int nmf_shade_mix_bwd(const float* V_rows, const float* f0_rows, const float* diffuse_rows,
                      const int32_t* cnt_rows, const int32_t* row_of_ray, int64_t R, const float* L,
                      const float* incoming, const float* brdf, const float* d_rows, float* d_incoming,
                      float* d_brdf, float* dL, float* d_f0diff, void* stream);
/* Same, plus dV [R][3] (nullable): the adjoint of the view direction per ray (F depends on V.H, H = normalize((V+L)/2)). */
int nmf_shade_mix_bwd_view(const float* V_rows, const float* f0_rows, const float* diffuse_rows,
                           const int32_t* cnt_rows, const int32_t* row_of_ray, int64_t R, const float* L,
                           const float* incoming, const float* brdf, const float* d_rows, float* d_incoming,
                           float* d_brdf, float* dL, float* d_f0diff, float* dV, void* stream);
/* RandHydraMLPDiffuse heads (modules/render_modules.py:519-574; pospe=-1, feape=0, one Linear each, std=0):
 * out [M][11] = (albedo 3 | tint 3 | f0 3 | roughness 2) with the activations applied; W [11][24] / b [11] are
 * the four Linear layers stacked in that order. */
int nmf_heads_fwd(const float* feat, int64_t M, const float* W, const float* b, float diffuse_mul,
                  float diffuse_bias, float tint_bias, float f0_bias, float rough_bias, float* out, void* stream);
/* d_feat [M][24] overwritten; gW [11][24], gb [11] ACCUMULATED (caller zeroes).  d_feat_add (may be NULL, may be d_feat
 * itself): another adjoint of the same rows, d_feat = d_feat_add + (this adjoint) -- the sum the caller would otherwise
 * spend a launch on. */
int nmf_heads_bwd(const float* feat, int64_t M, const float* W, const float* b, float diffuse_mul,
                  float diffuse_bias, float tint_bias, float f0_bias, float rough_bias, const float* d_out,
                  const float* d_feat_add, float* d_feat, float* gW, float* gb, void* stream);
/* Fused MLPBRDF (modules/brdf.py:177-261): out[r] = sigmoid(MLP(X[r])[0:3] + out_bias) with X as above and
 * MLP = Linear(66,64) ReLU Linear(64,64) ReLU Linear(64,4) (weights row-major [out][in], torch layout).
 * The dense layers run on v_mfma_f32_32x32x16_bf16 with every fp32 operand split into three bf16 terms (six products
 * per K block, fp32 accumulation: fp32-class accuracy, csrc/brdf_mlp.hip).  Writes out [R][3] and, when act_mask is not
 * NULL, the ReLU masks of the two hidden layers for the backward: act_mask [R][4] uint32 = per ray {layer-1 mask,
 * layer-2 mask} of lane half 0, then of lane half 1 (bit 16 ub + q = unit 32 ub + (q & 3) + 8 (q >> 2) + 4 half). */
int nmf_brdf_mlp_fwd(const void* image, const float* W0, const float* b0, const float* W2, const float* b2, const float* W4,
                     const float* b4, const float* half_vec, const float* diff_vec, const float* feat_src,
                     const float* rough_src, const int32_t* src_idx, int64_t R, float out_bias, float* out,
                     uint32_t* act_mask, int32_t max_workgroups /* 0 = default; see nmf_brdf_mlp_bwd_segments */, void* stream);
/* The weights of the forward and of the backward are given as the six tensors (image = NULL) or as a PACKED IMAGE (R4; W0..b4
 * are then not read): what the kernels stage into LDS in front of their first tile -- the split-bf16 planes of W0 | b0, W2
 * (forward: three terms; backward: two terms plus W2^T and W0[:, :24]^T) and the fp32 rows of the last layer -- written once per
 * weight update by nmf_brdf_mlp_pack (one launch of two workgroups) into nmf_brdf_mlp_image_bytes() bytes of device memory
 * (16-byte aligned).  A launch then starts with a byte copy instead of the conversion (the parameters are those of
 * modules/brdf.py:177-261's `self.mlp`, which change only in the optimizer step: train.py:733-735).  Results are bit-identical. */
int64_t nmf_brdf_mlp_image_bytes(void);
int nmf_brdf_mlp_pack(const float* W0, const float* b0, const float* W2, const float* b2, const float* W4, const float* b4,
                      void* image, int64_t image_bytes, void* stream);
/* Backward of nmf_brdf_mlp_fwd over ONE OR TWO ray sets in one launch (R4): the BRDF evaluations of a recursion level and of the
 * level below it (models/microfacet.py:377-456 at recur 0 and 1) share the weights, and a launch costs ~25 us before and after its
 * tiles whatever its size.  Sets with R = 0 are skipped.
 * Per set, the SAME inputs as the forward; fwd_out [R][3] and act_mask [R][4] are that call's outputs (the sigmoid adjoint and the
 * ReLU decisions come from them; the hidden activations are recomputed per 32-ray tile as values, two bf16 terms per operand).
 * d_feat [rows of feat_src][24] = adjoint of feat_src, ACCUMULATED (caller zeroes): the adjoints of the rays that gathered a row
 * (src_idx non-decreasing: consecutive rays) are summed inside the kernel, one atomic per (row, column) run of a 32-ray tile.
 * gW* / gb* are ACCUMULATED (caller zeroes): gW0 [64][66], gb0 [64], gW2 [64][64], gb2 [64], gW4 [4][64], gb4 [4] (row 3 of gW4 /
 * gb4 stays untouched: the fourth output is unused).
 * max_workgroups: 0 = the kernel's own choice (one persistent workgroup per CU, fewer for short launches); > 0 caps them, for
 * callers that run this launch on a second stream NEXT TO other kernels and want it to leave CUs free for them (the training
 * pass: nmf_amd/fast_step.py, csrc/step_core.inc).
 * workspace (device, nmf_brdf_mlp_bwd_segments_workspace_bytes(Rs, n_segs, max_workgroups) bytes, need not be initialised): one
 * partial sum of the weight gradients per workgroup; a second small launch adds them in workgroup order, so a gradient element
 * receives one atomic per call instead of one per workgroup. */
typedef struct nmf_mlp_bwd_segment {
    const float* half_vec;      /* [R][3] */
    const float* diff_vec;      /* [R][3] */
    const float* feat_src;      /* [rows][24] */
    const float* rough_src;     /* [rows] */
    const int32_t* src_idx;     /* [R] row of every ray, non-decreasing (NULL: ray r reads row r) */
    int64_t R;
    const float* fwd_out;       /* [R][3]  the forward's output */
    const uint32_t* act_mask;   /* [R][4]  the forward's ReLU masks */
    const float* d_out;         /* [R][3] */
    float* d_feat;              /* [rows][24], ACCUMULATED */
} nmf_mlp_bwd_segment;
int nmf_brdf_mlp_bwd_segments(const void* image, const float* W0, const float* b0, const float* W2, const float* b2,
                              const float* W4, const float* b4, const nmf_mlp_bwd_segment* segs /*HOST array*/, int32_t n_segs,
                              float* gW0, float* gb0, float* gW2, float* gb2, float* gW4, float* gb4, int32_t max_workgroups,
                              void* workspace, int64_t workspace_bytes, void* stream);
int64_t nmf_brdf_mlp_bwd_segments_workspace_bytes(const int64_t* Rs /*HOST*/, int32_t n_segs, int32_t max_workgroups);
/* out[s][0:D] = sum_{r in segment s} vals[r*row_stride + 0:D], D <= 64 (adjoint of the feature gather). */
int nmf_segment_sum_wide(const float* vals, int64_t row_stride, int32_t D, const int64_t* offsets,
                         int64_t n_seg, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Shading glue (csrc/shade.hip): the per-sample / per-ray spans between the big operators.
 * ---------------------------------------------------------------------------------------- */
/* models/microfacet.py:333-350.  counts [M] = secondary rays per sample (nmf_select_bounces).  Outputs:
 * bidx [>=Mb] samples with counts > 0 in order ("rows"), row_off [>=Mb+1] exclusive scan of their counts
 * (row_off[Mb] = R), cnt_rows [>=Mb] their counts, inv [M] row of each sample or -1, totals = {R, Mb}.
 * bidx / row_off / cnt_rows are sized by the caller for the worst case (M, M+1, M).
 * xyzt_rows (optional, [>=Mb][4], needs xyzt [M][4]): xyzt_rows[row] = xyzt[bidx[row]], the sample positions of the rows
 * (microfacet.py:352: `xyzs[bounce_mask]`), written by the same pass instead of a gather launch behind the size read-back.
 * M_live (DEVICE, may be NULL): the live element count when it is still on the device (e.g. totals[0] of nmf_march_scan); the
 * launch is sized by the bound M_cap, elements at or beyond *M_live are neither read nor written (see nmf_vm_query_fwd).
 * publish_mapped_dev (may be NULL): [R, Mb, publish_seq] is also published into mapped host memory (see nmf_march_scan). */
int nmf_bounce_index(const int32_t* counts, int64_t M_cap, const int64_t* M_live, int32_t* bidx, int64_t* row_off,
                     int32_t* cnt_rows, int32_t* inv, int64_t* totals, const float* xyzt, float* xyzt_rows, void* workspace,
                     int64_t workspace_bytes, void* publish_mapped_dev, int64_t publish_seq, void* stream);
int64_t nmf_bounce_index_workspace_bytes(int64_t M);
/* nmf_select_bounces + nmf_bounce_index in the launches of the latter (R4): the bounce count of a sample is one expression
 * of (weights[i], u[i]) (modules/pt_selectors.py:5-60; arguments as nmf_select_bounces), evaluated inside the index kernels
 * instead of by a launch of its own on the forward's chain.  counts are not materialised.  M_cap <= 2^20; M_live may be NULL. */
int nmf_bounce_index_select(const float* weights, const float* u, int32_t mode, float mul, float add, float sum_w,
                            const float* sum_w_dev, int64_t M_cap, const int64_t* M_live, int32_t* bidx, int64_t* row_off,
                            int32_t* cnt_rows, int32_t* inv, int64_t* totals, const float* xyzt, float* xyzt_rows,
                            void* workspace, int64_t workspace_bytes, void* publish_mapped_dev, int64_t publish_seq,
                            void* stream);
/* Per bounce row (models/microfacet.py:297,304-316,352-361): V = -ray direction, N = normal facing V
 * (n * sign(V.n)), r1 = max(roughness, min_rough), f0, diffuse = albedo * E(n) with E the 9-term SH irradiance
 * (conv [9][3] DEVICE pointer, modules/sh.py:97-142), feat = app + anoise * feat_noise (feat_noise may be NULL),
 * xyz.  heads is nmf_heads_fwd's output, rays [b][6], ray_id [M].  app / heads / feat_noise are indexed by SAMPLE
 * ([M][24], [M][11], [M][24]) or, with row_inputs != 0, by BOUNCE ROW ([Mb][.]: appearance evaluated only where it is
 * used -- in training that is ~5-20 % of the samples).  row_inputs == 2: `normals` is indexed by bounce row as well
 * ([Mb][3]: below the first recursion level normals are only needed where secondary rays start). */
int nmf_bounce_prep_fwd(const int32_t* bidx, int64_t Mb, const float* normals, const float* app, const float* heads,
                        const float* xyzt, const int32_t* ray_id, const float* rays, const float* conv,
                        const float* feat_noise, float anoise, float min_rough, int32_t row_inputs, float* V, float* N,
                        float* r1, float* f0, float* diffuse, float* feat, float* xyz, void* stream);
/* The same with the material heads evaluated inside the launch (R4): head_W [11][24], head_b [11] and the five activation
 * parameters of nmf_heads_fwd instead of its output; heads_out [Mb][11] receives what nmf_heads_fwd(app) would have written (the
 * backward reads it).  app must be given per bounce row (row_inputs 1 or 2).  One launch less per recursion level on the
 * forward's chain; the same bits as nmf_heads_fwd followed by nmf_bounce_prep_fwd. */
int nmf_bounce_prep_fwd_heads(const int32_t* bidx, int64_t Mb, const float* normals, const float* app, const float* head_W,
                              const float* head_b, float diffuse_mul, float diffuse_bias, float tint_bias, float f0_bias,
                              float rough_bias, const float* xyzt, const int32_t* ray_id, const float* rays, const float* conv,
                              const float* feat_noise, float anoise, float min_rough, int32_t row_inputs, float* heads_out,
                              float* V, float* N, float* r1, float* f0, float* diffuse, float* feat, float* xyz, void* stream);
/* Adjoint: d_normals [M][3] written for ALL samples (zeros where inv < 0 or detach_normals); d_heads / d_app written for
 * all M samples ([M][11], [M][24], zeros where inv < 0) or, with row_inputs, per bounce row ([Mb][11], [Mb][24]; bidx
 * required); row_inputs == 2: normals AND d_normals are per bounce row ([Mb][3]), inv is not read.  Row gradients may be
 * NULL (= zero).  row_strides = row pitch in floats of (dN, dr1, df0, ddiffuse), so
 * column slices of wider row tensors are read in place (NULL = dense 3,1,3,3). */
int nmf_bounce_prep_bwd(const int32_t* inv, int64_t M, const int32_t* bidx, int64_t Mb, const float* normals,
                        const float* heads, const int32_t* ray_id, const float* rays, const float* conv,
                        float min_rough, int32_t detach_normals, int32_t row_inputs, const float* dN,
                        const float* dr1, const float* df0,
                        const float* ddiffuse, const int32_t row_strides[4], const float* dfeat, float* d_normals,
                        float* d_heads, float* d_app, void* stream);
/* nmf_bounce_prep_bwd (everything per bounce row: row_inputs = 2) + nmf_heads_bwd in ONE launch (R4): the adjoint of the heads'
 * outputs and the feature-row adjoint that nmf_heads_bwd adds are computed per row from the inputs of nmf_bounce_prep_bwd instead
 * of written and read back.  d_normals [Mb][3], d_app [Mb][24] (the adjoint of `app`: heads' backward + dfeat); g_head_W / g_head_b
 * ACCUMULATED as in nmf_heads_bwd.  One launch less per recursion level on the backward's main chain. */
int nmf_bounce_prep_heads_bwd(const int32_t* bidx, int64_t Mb, const float* normals, const float* heads, const int32_t* ray_id,
                              const float* rays, const float* conv, float min_rough, int32_t detach_normals, const float* dN,
                              const float* dr1, const float* df0, const float* ddiffuse, const int32_t row_strides[4],
                              const float* dfeat, const float* app, const float* head_W, const float* head_b, float diffuse_mul,
                              float diffuse_bias, float tint_bias, float f0_bias, float rough_bias, float* d_normals, float* d_app,
                              float* g_head_W, float* g_head_b, void* stream);
/* modules/tensor_nerf.py:448-452,583-587,658-659 + modules/tonemap.py:34-55, one thread per ray in sample order:
 * acc = sum w, rgb_lin = sum w * refl_rows[inv], ori = sum w * min(-d.n, 0)^2 (ori / normals may be NULL),
 * rgb_map = (tonemap ? srgb(rgb_lin) : rgb_lin) + (1 - acc) * bg;  bg [3] or [B][3] (bg_per_ray). */
int nmf_ray_compose_fwd(const float* weight, const float* refl_rows, const int32_t* inv, const float* normals,
                        const float* rays, const int64_t* offsets, int64_t B, const float* bg, int32_t bg_per_ray,
                        int32_t tonemap, int32_t noclip, float* rgb_map, float* acc, float* rgb_lin, float* ori,
                        void* stream);
/* Adjoint, one thread per sample: d_weight [M], d_refl [Mb][3] (every row written), d_normals [M][3] (may be NULL).
 * d_rgb_map [B][3], d_acc [B], d_ori [B] may each be NULL.  The background gradient (1 - acc) * d_rgb_map is
 * left to the caller. */
int nmf_ray_compose_bwd(const float* weight, const float* refl_rows, const int32_t* inv, const float* normals,
                        const float* rays, const int32_t* ray_id, int64_t M, const float* bg, int32_t bg_per_ray,
                        int32_t tonemap, int32_t noclip, const float* rgb_lin, const float* d_rgb_map,
                        const float* d_acc, const float* d_ori, float* d_weight, float* d_refl, float* d_normals,
                        void* stream);
/* ... which is this: d_bg [B][3] = (1 - acc[B]) * d_rgb_map [B][3] (tensor_nerf.py:658-659 backward for a per-ray
 * background: the adjoint handed to nmf_sat_lookup_bwd). */
int nmf_bg_adjoint(const float* acc, const float* d_rgb_map, int64_t B, float* d_bg, void* stream);

/* Retrace selection (models/microfacet.py:475-537, csrc/retrace.hip).
 * score[r] = max_c(brdf[r][c]) * [V.N > 0 of the ray's row] * exp(lpdf[r]) * w_rows[row] / (cnt_rows[row] + 1e-8). */
int nmf_retrace_scores(const float* brdf /*[R][3]*/, const float* V_rows, const float* N_rows /*[Mb][3]*/,
                       const float* lpdf /*[R]*/, const float* w_rows /*[Mb]*/, const int32_t* cnt_rows,
                       const int32_t* row_of_ray, int64_t R, float* score, void* stream);
/* order = argsort(keys) ascending (= torch.argsort of microfacet.py:522; ties in unspecified order), radix sort of
 * (key, index) pairs on the caller's workspace. */
int nmf_argsort_f32(const float* keys, int64_t n, int32_t* order, void* workspace, int64_t workspace_bytes,
                    void* stream);
/* The partition the reference takes from that argsort (models/microfacet.py:506-537: retrace_ray_inds = cc_as[M:], notrace_ray_inds =
 * cc_as[:M]) WITHOUT sorting all n keys: a radix select (three histogram passes of 11 / 11 / 10 bits over the keys find the key of ascending rank
 * n - k; ties at the cut go the way a stable ascending sort places them).  idx_top [k] = argsort(keys)[n-k:] exactly, in that order
 * (the re-traced rays are processed in it); idx_rest [n-k] = the indices of argsort(keys)[:n-k] in INDEX order (their order is never
 * used).  Either output may be NULL when empty. */
int64_t nmf_topk_select_workspace_bytes(int64_t n);
int nmf_topk_select(const float* keys, int64_t n, int64_t k, int32_t* idx_top, int32_t* idx_rest, void* workspace,
                    int64_t workspace_bytes, void* stream);
int64_t nmf_argsort_workspace_bytes(int64_t n);

/* ------------------------------------------------------------------------------------------
 * Loss terms (csrc/loss.hip).  `out` scalars are ACCUMULATED into (caller zeroes).
 * ---------------------------------------------------------------------------------------- */
/* fields/tensoRF.py:332-340 density_L1: out += sum_i mean(|x_i|) over up to 8 dense fp32 tensors (x, numel: HOST arrays
 * of `count` entries); backward g_i = d_out * sgn(x_i) / numel_i, written in x_i's own memory order -- or, with
 * accumulate != 0, ADDED to g_i (which then already holds the rendering gradient of the same factor: one launch instead
 * of one accumulation kernel per tensor). */
int nmf_l1_mean_fwd(const float* const x[], const int64_t numel[], int32_t count, float* out, void* stream);
int nmf_l1_mean_bwd(const float* const x[], const int64_t numel[], int32_t count, const float* d_out,
                    float* const g[], int32_t accumulate, void* stream);
/* train.py:598-601 photometric term: out += sum (clip(pred,0,1) - clip(gt,0,1))^2 over n floats; backward
 * d_pred = 2 (pred - clip(gt)) d_out inside [0,1], 0 outside (d_out: device scalar). */
int nmf_sqerr_fwd(const float* pred, const float* gt, int64_t n, float* out, void* stream);
int nmf_sqerr_bwd(const float* pred, const float* gt, int64_t n, const float* d_out, float* d_pred, void* stream);
/* train.py:640-677 loss assembly: out += scale * sum_i w_i * sum(x_i) over up to 8 dense fp32 tensors (scalars or
 * per-ray vectors such as the orientation terms of tensor_nerf.py:583-587 and acc_map of :598-602); backward fills
 * g_i[:] = d_out * scale * w_i (d_out: device scalar).  x, numel, w, g: HOST arrays of `count` entries. */
int nmf_loss_mix_fwd(const float* const x[], const int64_t numel[], const float w[], int32_t count, float scale,
                     float* out, void* stream);
int nmf_loss_mix_bwd(const int64_t numel[], const float w[], int32_t count, float scale, const float* d_out,
                     float* const g[], void* stream);
/* The head of a training chunk's backward in ONE launch (train.py:598-601 + 640-677; the same values as nmf_sqerr_fwd +
 * nmf_loss_mix_bwd + nmf_sqerr_bwd, which stay for callers that need the pieces): loss[0] = sum (clip(pred,0,1) -
 * clip(gt,0,1))^2 over [n_rays][3], WRITTEN (per-workgroup sums added in workgroup order by the workgroup that finishes
 * last: no zero fill, no float atomics, run-to-run identical); d_pred = 2 (pred - clip(gt)) * (d_out scale w_pred) inside
 * [0,1], 0 outside; g_a / g_b [n_rays] (each may be NULL) filled with d_out scale w_a / w_b (the constant adjoints of the
 * per-ray acc / orientation terms).  d_out: device scalar.  workspace: nmf_loss_head_workspace_bytes(n_rays) bytes, 16-byte
 * aligned, whose first 4 bytes are ZERO before the first use (a ticket counter the launch leaves at zero again); one
 * workspace serves one stream at a time. */
int64_t nmf_loss_head_workspace_bytes(int64_t n_rays);
int nmf_loss_head(const float* pred, const float* gt, int64_t n_rays, const float* d_out, float scale, float w_pred,
                  float w_a, float w_b, float* loss, float* d_pred, float* g_a, float* g_b, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer: torch.optim.Adam over the per-module param groups (train.py:443-469), every tensor in one launch.
 * `slots` is a HOST array (copied into kernel arguments); hyper-parameters per slot are the group's, with the
 * bias corrections computed by the host in double precision exactly as torch/optim/adam.py does:
 *   step_size = lr / (1 - beta1^t),  bc2_sqrt = sqrt(1 - beta2^t).
 * param/grad/exp_avg/exp_avg_sq share one dense layout of `numel` elements (fp32, or fp64 when is_f64).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    void* param;
    const void* grad;
    void* exp_avg;
    void* exp_avg_sq;
    int64_t numel;
    double beta1, beta2, eps, weight_decay, step_size, bc2_sqrt;
    int32_t is_f64;
    int32_t reserved;
} nmf_adam_slot;
/* guard (DEVICE, may be NULL): the update is gated by that float (e.g. the summed loss of the step): not finite -> no parameter and
 * no moment changes.  train.py:704-705 skips a chunk whose loss is NaN after a host read-back; this keeps the decision on the device. */
int nmf_adam_step(const nmf_adam_slot* slots, int32_t n_slots, const float* guard, void* stream);

/* Multi-tensor copy with fp32 <-> fp64 conversion, all slots in one launch (slots: HOST array, passed by value): packs the
 * per-parameter gradients into the flat fp32 all-reduce buffer and unpacks the reduced sums (ONE collective
 * per optimizer step).  src / dst are dense runs of `numel` elements. */
typedef struct {
    const void* src;
    void* dst;
    int64_t numel;
    int32_t src_is_f64;      /* 0: fp32 source, 1: fp64 source */
    int32_t dst_is_f64;      /* 0: fp32, 1: fp64, 2: bfloat16 (fp32 source only, round to nearest even) */
} nmf_copy_slot;
int nmf_multi_copy(const nmf_copy_slot* slots, int32_t n_slots, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation metrics of renderer.py:195-560 (evaluate).  Not on the training path; deterministic (fp64 partial sums per
 * workgroup in the workspace, summed per view in a fixed order by a second launch: no float atomics), so a view's value is
 * bit-identical from run to run and independent of how many views share a call.  n_img == 0 is a no-op.
 *
 * nmf_ssim: utils.py:90-136 (rgb_ssim) for filter_size 11.  a, b: contiguous [n_img][H][W][C] fp32, C == 3, H, W >= 11.
 * taps11: HOST array of the 11 normalised Gaussian taps (fp64, utils.py:101-106), read at call time.  c1 = (k1 max_val)^2,
 * c2 = (k2 max_val)^2.  Moments and the per-pixel formula in fp64 (valid-mode separable filter, sigma00 / sigma11 clamped at
 * 0, sigma01 limited to sign * min(sqrt(sigma00 sigma11), |sigma01|)).  mean_out [n_img] fp64: the mean of the map over pixels
 * and channels; map_out [n_img][H-10][W-10][C] fp32 or NULL.  workspace >= nmf_ssim_workspace_bytes(n_img, H, W, C).
 * ---------------------------------------------------------------------------------------- */
int nmf_ssim(const float* a, const float* b, int64_t n_img, int32_t H, int32_t W, int32_t C,
             const double* taps11, double c1, double c2,
             double* mean_out, float* map_out, void* workspace, int64_t workspace_bytes, void* stream);
int64_t nmf_ssim_workspace_bytes(int64_t n_img, int32_t H, int32_t W, int32_t C);
/* nmf_normal_err: renderer.py:369-389 per view.  pred, gt: [n_img][n_px][3] fp32 normals, acc: [n_img][n_px] fp32 alpha.
 * Per pixel in fp32 in the torch expression's order: q = (n*127 + 128) truncated toward zero, (q - 128) / 127, divided by
 * sqrt(sum n^2 + 1e-6), dot clipped to [1e-8, 1] (1 - 1e-8 is 1 in fp32), acos * 180 / pi, NaN (or a non-finite normal) -> 0,
 * times acc.  mean_out [n_img] fp64 = sum(err * acc) / sum(acc) (NaN when sum(acc) == 0, as the reference); err_map
 * [n_img][n_px] fp32 (err * acc, what the reference writes to normal_err/) or NULL.
 * workspace >= nmf_normal_err_workspace_bytes(n_img, n_px). */
int nmf_normal_err(const float* pred, const float* gt, const float* acc, int64_t n_img, int64_t n_px,
                   double* mean_out, float* err_map, void* workspace, int64_t workspace_bytes, void* stream);
int64_t nmf_normal_err_workspace_bytes(int64_t n_img, int64_t n_px);

/* ------------------------------------------------------------------------------------------
 * Material maps of the evaluation pass (renderer.py:440-463, modules/tensor_nerf.py:480-566, models/microfacet.py:299-316,
 * 572,615-672), recursion level 0.  Per primary ray r with kept samples k = offsets[r] .. offsets[r+1]-1:
 *   map_X[r] = sum_k w_k X_k + (1 - acc[r]) bg
 * with h = heads(app_k) (the 24 -> 11 heads of nmf_heads_fwd, no feature noise), n = normals[k], v = rays[r][3:6] and
 *   albedo    = h[0:3]
 *   roughness = h[9] (one value, the bg term makes it 3 channels)
 *   diffuse   = (1 - Fr) albedo E,  E[c] = sum_j conv[j][c] Y_j(n) (the 9 SH bases of modules/sh.py)
 *   tint      = Fr brdf_rgb_k
 *   spec      = spec_k
 *   Fr = f0 + (1 - f0) clip(1 - |dot(-v, n)|, 0, 1)^5, f0 = h[6:9]
 * For a sample with a bounce row q = inv[k] >= 0, spec_k / brdf_rgb_k = sum over the rays j = row_off[q] .. row_off[q+1]-1 of
 * incoming[j] / max(cnt[q], 1) and brdf_weight[j] / max(cnt[q], 1) (index order); 0 for every other sample.
 * app [M][24], normals [M][3], weight [M], offsets [B+1] int64, rays [B][6], head_W [11][24], head_b [11], conv [9][3],
 * inv [M] int32 (bounce row or -1), row_off [Mb+1] int64, cnt [Mb] int32, incoming / brdf_weight [R][3], acc [B], bg [3] (device).
 * Mb == 0 (then R == 0): the row inputs may be NULL, spec and tint are 0.
 * out [B][15] fp32: albedo 0-2 | roughness 3-5 | diffuse 6-8 | tint 9-11 | spec 12-14.  One launch; a lane group per ray sums its
 * samples in a fixed order (bit-identical from run to run); samples with w == 0 are skipped; no per-sample value is stored.
 * ---------------------------------------------------------------------------------------- */
int nmf_material_maps(const float* app, const float* normals, const float* weight, const int64_t* offsets, int64_t B, int64_t M,
                      const float* rays, const float* head_W, const float* head_b, float diffuse_mul, float diffuse_bias,
                      float tint_bias, float f0_bias, float rough_bias, const float* conv, const int32_t* inv,
                      const int64_t* row_off, const int32_t* cnt, int64_t Mb, const float* incoming, const float* brdf_weight,
                      int64_t R, const float* acc, const float* bg, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Material edits: the heads' outputs changed at render time (evaluation only; nothing here has a backward).
 * An edit list holds n_edits <= NMF_EDIT_MAX edits, applied in list order, each to the result of the one before.  An edit sees
 * a sample's world position x (the frame of aabb and of the exported mesh) and its 11 head outputs v (nmf_heads_fwd).
 *   target     albedo v[0:3] | f0 v[6:9] | roughness v[9] and v[10] (both alike).  The tint head v[3:6] is not editable.
 *   region     all:        mask 1
 *              box:        centre c, half extents h, d = max_i(|x_i - c_i| - h_i)
 *              ellipsoid:  centre c, radii h, q_i = (x_i - c_i) / h_i, d = (sqrt((q0 q0 + q1 q1) + q2 q2) - 1) min(h)
 *   mask       falloff == 0: m = d <= 0 ? 1 : 0;  falloff > 0: s = clamp(1 - d / falloff, 0, 1), m = (s s)(3 - 2 s);
 *              invert: m = 1 - m
 *   operator   colour targets: t_c = ((A_c0 v_0 + A_c1 v_1) + A_c2 v_2) + b_c, clamped to [0, 1]
 *              roughness:      t_j = A_00 v_j + b_0, clamped to [0.01, 1] (the head's own clip)
 *   blend      m == 0: the value keeps its bits;  m == 1: out = t;  otherwise out = v + m (t - v)
 * fp32 with one rounding per operation in the order written, no fma: a float32 restatement that follows the same order gives the
 * same bits (nmf_amd/edit.py apply_reference), and an identity edit (A = I, b = 0) returns its input bits.
 *
 * The table `edits` is HOST memory, [n_edits][NMF_EDIT_ROW] fp32; it is checked and then travels in the kernel arguments:
 *   0 kind (0 all, 1 box, 2 ellipsoid) | 1 target (0 albedo, 1 f0, 2 roughness) | 2 invert (0 / 1) | 3 falloff | 4-6 c | 7-9 h |
 *   10-18 A row-major | 19-21 b | 22-31 zero
 * Checked before anything is launched: n_edits > NMF_EDIT_MAX, an entry that is not finite, a kind / target / invert outside the
 * values above, falloff < 0, h <= 0 for a box or an ellipsoid: NMF_ERANGE.  Null pointers, negative sizes, xyz_stride other than
 * 3 or 4: NMF_EINVAL.
 *
 * nmf_heads_edit: heads [n][11] (device) edited in place; xyz [n][xyz_stride] (device; 4: the xyzt rows the passes carry, the
 * fourth column is not read).  n == 0 or n_edits == 0: nothing is launched.  One launch: a lane per row, a workgroup's 256 rows
 * moved through LDS with coalesced dword accesses.
 * nmf_material_maps_edit: nmf_material_maps with the edits applied to every sample's head outputs right after they are evaluated
 * (xyz [M][xyz_stride]: the samples' positions).  n_edits == 0: the launch and the bits of nmf_material_maps (xyz may be NULL).
 * ---------------------------------------------------------------------------------------- */
#define NMF_EDIT_ROW 32
#define NMF_EDIT_MAX 16
int nmf_heads_edit(float* heads, const float* xyz, int32_t xyz_stride, int64_t n, const float* edits, int32_t n_edits, void* stream);
int nmf_material_maps_edit(const float* app, const float* normals, const float* weight, const int64_t* offsets, int64_t B, int64_t M,
                           const float* rays, const float* head_W, const float* head_b, float diffuse_mul, float diffuse_bias,
                           float tint_bias, float f0_bias, float rough_bias, const float* conv, const int32_t* inv,
                           const int64_t* row_off, const int32_t* cnt, int64_t Mb, const float* incoming, const float* brdf_weight,
                           int64_t R, const float* acc, const float* bg, float* out, const float* xyz, int32_t xyz_stride,
                           const float* edits, int32_t n_edits, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh export: indexed marching cubes over a dense volume (the reference's scripts/export_mesh.py runs
 * skimage.measure.marching_cubes on the host through utils.convert_sdf_samples_to_ply).  Not on the training path.
 * vol [gx][gy][gz] fp32, C order (what AlphaGridSampler.getDenseAlpha returns), every axis 2..1024 points (else NMF_ERANGE), flat
 * indices int64.  A lattice point is inside when vol > level; a NaN is outside.
 *
 * One vertex per lattice edge whose two ends differ in insideness, owned by the lattice point n = (i gy + j) gz + k at the edge's
 * lower end (a point owns its +x, +y, +z edges, in this order).  Position along the edge's axis, in lattice index units, fp32 with
 * one rounding per operation: p = i + (level - a) / (b - a), a = vol at the owner, b = vol at the other end (a NaN or infinite
 * end gives a NaN coordinate).  Faces are int32 triples of vertex indices; their normals point from inside to outside (a closed
 * blob has a positive signed volume sum(det[p0, p1, p2]) / 6, the reference's orientation after its faces[..., ::-1]).
 *
 * Cases: corner c = dx + 2 dy + 4 dz of the cell at n, bit c of the case byte = that corner is inside; corners past the volume
 * repeat the last point of their axis (the points of the upper faces own edges but no triangles).  Edge e = 4 axis + k runs along
 * axis (0 x, 1 y, 2 z) from the corner whose two other coordinates are (k & 1, k >> 1), in the order of the remaining axes.
 * The 256-case table (csrc/mc_table.hpp) is generated by tools/gen_mc_table.py; on a face with four crossings every inside corner is
 * cut off by its own segment, a rule of the face's four signs only, so neighbouring cells agree (no holes).
 *
 * nmf_mc_count: cases [N] uint8, vcount [N] int32 (owned vertices, 0..3), tcount [N] int32 (triangles, 0..5), N = gx gy gz, in
 * lattice order.  The caller replaces vcount / tcount by their INCLUSIVE sums in that order (in place: the scan is plumbing, e.g.
 * torch.cumsum), reads back the two totals V and F and allocates verts [V][3] fp32 and faces [F][3] int32.
 * nmf_mc_emit: point n writes its vertices from vscan[n - 1] and its faces from tscan[n - 1] (0 for n == 0); a face finds a
 * neighbour's vertex through that neighbour's case byte and scanned base.  No atomics: the output order is the lattice order, two
 * runs give identical bytes.  NMF_ERANGE if n_verts or 3 n_faces passes 2^31 - 1.  Stores are checked against n_verts / n_faces.
 * V == 0 and F == 0: no launch, verts / faces may be NULL.  One launch each.
 * nmf_mc_workspace_bytes: 9 bytes per lattice point (cases + vcount + tcount), the working memory beyond the volume and the
 * outputs; 0 for a non-positive size.  Host arithmetic.
 * nmf_mc_case_triangles: host only.  Writes the edge triples of one case (-1 padded) and returns its triangle count (0..5), or a
 * negative code.
 * ---------------------------------------------------------------------------------------- */
int nmf_mc_count(const float* vol, int32_t gx, int32_t gy, int32_t gz, float level, uint8_t* cases, int32_t* vcount,
                 int32_t* tcount, void* stream);
int nmf_mc_emit(const float* vol, int32_t gx, int32_t gy, int32_t gz, float level, const uint8_t* cases, const int32_t* vscan,
                const int32_t* tscan, int64_t n_verts, int64_t n_faces, float* verts, int32_t* faces, void* stream);
int64_t nmf_mc_workspace_bytes(int32_t gx, int32_t gy, int32_t gz);
int nmf_mc_case_triangles(int case_index, int8_t out[16]);

/* ------------------------------------------------------------------------------------------
 * Total-variation regularisers (utils.py:139-151 TVLoss on the VM planes / lines, modules/integral_equirect.py:399-407 tv_loss on
 * the environment map; train.py:684-709 adds them to every chunk's loss).  `count` (1..16) tensors in ONE launch:
 *   value_out[0] = scale * sum_i w[i] * TV_i(x_i)                       (WRITTEN; NULL: gradient only)
 *   g[i]        += scale * w[i] * dTV_i/dx_i                            (ADDED;   g == NULL: value only)
 * shape [count][3] = (C, H, W) of x_i[1][C][H][W]; x_stride / g_stride [count][3]: element strides along C, H, W of x_i / g_i --
 * any dense storage order (the field's tables are channel-last, a gradient accumulator may differ from its parameter), else
 * NMF_EINVAL.  kind[i]:
 *   NMF_TV_PLANE  mean over c, h < H-1, w < W-1 of sqrt(dw^2 + dh^2 + 1e-5), dh = x[h+1][w] - x[h][w], dw = x[h][w+1] - x[h][w];
 *                 H < 2 or W < 2: NMF_ERANGE (the reference's mean over an empty set is NaN)
 *   NMF_TV_LINE   W == 1: mean |x[g+1] - x[g]|, sign(0) = 0 in the gradient; H < 2: NMF_ERANGE
 *   NMF_TV_ENVMAP C == 3, the reference's arithmetic on bg_mat[0] = [3][H][W] AS WRITTEN: mean over c < 2, h < H-1, all w of
 *                 |x[c+1][h][w] - x[c][h][w]| + |x[c][h+1][w] - x[c][h][w]| + 1e-8; H < 2: NMF_ERANGE
 * Terms and gradient in fp32 without contraction, the value as the fp64 sum of the terms: per-workgroup sums added in workgroup
 * order by the workgroup that finishes last (no zero fill, no float atomics: run-to-run and stream-to-stream identical).  The
 * gradient is a gather (each element's own term and its lower neighbours' terms): no atomics.  scale_dev: device scalar.
 * workspace (only read with value_out): nmf_tv_workspace_bytes(shape, kind, count) bytes (or a negative code for a refused table),
 * 16-byte aligned, whose first 4 bytes are ZERO before the first use (the ticket, left at zero again); one workspace serves one
 * stream at a time.  A refused call launches nothing and writes nothing. */
#define NMF_TV_PLANE 0
#define NMF_TV_LINE 1
#define NMF_TV_ENVMAP 2
int64_t nmf_tv_workspace_bytes(const int32_t* shape, const int32_t* kind, int32_t count);
int nmf_tv_fwd_bwd(const float* const x[], float* const g[], const int32_t* shape, const int64_t* x_stride, const int64_t* g_stride,
                   const int32_t* kind, const float w[], int32_t count, const float* scale_dev, float* value_out, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Relighting: a spherical radiance function resampled into an IntegralEquirect texel grid under a rotation (no reference
 * counterpart as a function: scripts/car_rotating_lights.ipynb rotates lights in a notebook, scripts/pano2cube.py imports a
 * panorama by fitting).  dst [3][H][W] (a bg_mat) = log(max(gain * mean of supersample^2 stratified sub-samples of the texel's
 * extent, 1e-8)); a NaN becomes the floor.  Texel (i, j) covers ix in (j - 1, j], iy in (i - 1, i] of the summed-area table's
 * coordinates, each sub-sample becomes a direction d, and the source is read along R^T d (row-major R = r00..r22:
 * the lighting rotated by R), bilinearly, in LINEAR radiance:
 *   kind 0  src [3][Hs][Ws], the activated table of a module map (nmf_sat_build's `activated`): texel centres at ix = j - 1/2,
 *           columns periodic over 1..Ws-1, rows clamped to 1..Hs-1
 *   kind 1  src [Hs][Ws][3], a panorama in pano2env.pixel_directions' parameterisation (scripts/pano2cube.py:101-109): columns
 *           periodic with period Ws - 1, rows clamped
 * One thread per destination texel, no atomics: the same bytes on every run.  Refused (nothing launched): a null pointer or a size
 * below 4, an unknown kind, a gain that is not finite and positive, max|R^T R - I| > 1e-4 (NMF_EINVAL); supersample outside 1..8
 * (NMF_ERANGE). */
int nmf_env_resample(const float* src, int32_t kind, int32_t Hs, int32_t Ws, float r00, float r01, float r02, float r10, float r11,
                     float r12, float r20, float r21, float r22, float gain, int32_t supersample, float* dst, int32_t H, int32_t W,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Relighting evaluation: the pixel arithmetic of scripts/relighting_calc.ipynb and of the HDR frame renderer.py:425-429 stores
 * (nmf_amd/relight_eval.py).  Images are n_img x H x W pixels, P = H W.  srgb / srgb_inverse are
 * modules/tonemap.py:38-55 (forward limit 0.0031308 with max(x, limit) under the power, inverse limit 0.04045).
 *
 * nmf_relight_frame: rgb_lin [n_img][P][3] (the composited radiance sum_k w_k c_k of nmf_ray_compose_fwd), acc [n_img][P] ->
 *   out [n_img][P][3] = srgb_inverse(srgb_noclip(rgb_lin) + (1 - acc)).
 * nmf_relight_ratio: pred [n_img][P][3], gt [n_img][P][4] (RGBA, 16-byte aligned) -> sum [n_img][3] (double), the sum of
 *   gt_c / max(pred_c, 1e-7) (an fp32 quotient, added in double) over the pixels with gt_a > 0.5 and min_c pred_c > 0.01 (both
 *   strict), and count [n_img] (int64), the number of those pixels.
 * nmf_relight_adjust: tp [n_img][P][3] = clip(srgb((pred_c * multi_c) * gt_a + (1 - gt_a)), 0, 1), tg [n_img][P][3] =
 *   clip(srgb(gt_c + (1 - gt_a)), 0, 1), sqerr [n_img] (double) = sum over pixels and channels of the fp32 (tp - tg)^2.
 * workspace (16-byte aligned) >= the matching *_workspace_bytes(n_img, H, W) (0 for sizes the call refuses); its content before the
 * call does not matter.  No atomics: per-workgroup partials added in workgroup order, the same bytes on every run.  Refused (nothing
 * launched): a null pointer, n_img, H or W below 1, a misaligned gt / workspace, a workspace that is too small, a multiplier that is
 * not finite (NMF_EINVAL); more pixels than one call's grid covers (NMF_ERANGE). */
int nmf_relight_frame(const float* rgb_lin, const float* acc, int64_t n_img, int64_t H, int64_t W, float* out, void* stream);
int64_t nmf_relight_ratio_workspace_bytes(int64_t n_img, int64_t H, int64_t W);
int nmf_relight_ratio(const float* pred, const float* gt, int64_t n_img, int64_t H, int64_t W, double* sum, int64_t* count,
                      void* workspace, int64_t workspace_bytes, void* stream);
int64_t nmf_relight_adjust_workspace_bytes(int64_t n_img, int64_t H, int64_t W);
int nmf_relight_adjust(const float* pred, const float* gt, float multi_r, float multi_g, float multi_b, int64_t n_img, int64_t H,
                       int64_t W, float* tp, float* tg, double* sqerr, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Camera paths: the two per-frame kernels around the evaluation pass (nmf_amd/renderer.py:evaluation_path).
 *
 * nmf_camera_rays: the pixel rays of a pinhole camera from its camera-to-world matrix (row-major 3x4: rotation r00..r22, translation
 *   tx ty tz; OpenCV axes, x right, y down, z forward), as the loader builds them on the host for every view of a data set
 *   (dataLoader/ray_utils.py:23-41, 65-85; dataLoader/blender.py:97-122).  rays [H W][6] = origin | unit direction, pixel
 *   p = row W + col.  fp32, one rounding per operation, in this order:
 *     x = ((col + 0.5) - cx) / fx,  y = ((row + 0.5) - cy) / fy,  n = sqrt((x x + y y) + 1),  d = (x / n, y / n, 1 / n),
 *     world_i = (r_i0 d_x + r_i1 d_y) + r_i2 d_z,  origin = (tx, ty, tz).
 *   fx != fy and an off-centre principal point are allowed.  One launch, one lane per pixel; two runs give the same bytes.  Refused
 *   (nothing launched): a null or not 8-byte aligned rays, H or W below 1, fx or fy zero or not finite, a pose, cx or cy that is not
 *   finite (NMF_EINVAL); H W above 2^31 - 1 (NMF_ERANGE).
 *
 * nmf_frame_finish: the float maps of one frame -> one 8-bit picture ready to encode.  Each non-null input is one panel, side by side
 *   in the order rgb [P][3] | depth [P] | normal [P][3] | acc [P], P = H W: panel k of pixel (row, col) is the three bytes at
 *   out[((row n_panels + k) W + col) 3].  Per value, a NaN counts as 0 before anything else; the casts truncate:
 *     rgb     (uint8)(clamp(v, 0, 1) * 255)                                         (renderer.py:343-347, after a clip to [0, 1])
 *     depth   q = (uint8)(255 clamp((v - near) / ((far - near) + 1e-8f), 0, 1)); the pixel is lut[q] (lut [256][3] bytes), or
 *             (q, q, q) when lut is NULL          (utils.visualize_depth_numpy with minmax = near_far, clamped instead of wrapped)
 *     normal  (uint8)clamp(v * 127 + 128, 0, 255)                                   (renderer.py:440-451, vis_world_normal)
 *     acc     (uint8)(255 clamp(v, 0, 1)), grey
 *   One launch; a lane owns four consecutive output pixels and stores three dwords when out is 4-byte aligned, bytes otherwise and in
 *   the tail.  Refused (nothing launched): all four inputs null, a null out, H or W below 1, near or far not finite, far <= near
 *   (NMF_EINVAL); H W n_panels above 2^31 - 1 (NMF_ERANGE). */
int nmf_camera_rays(float r00, float r01, float r02, float r10, float r11, float r12, float r20, float r21, float r22, float tx,
                    float ty, float tz, float fx, float fy, float cx, float cy, int32_t H, int32_t W, float* rays, void* stream);
int nmf_frame_finish(const float* rgb, const float* depth, const float* normal, const float* acc, float near, float far,
                     const uint8_t* lut, int32_t H, int32_t W, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Texture atlas of an exported mesh: one chart per triangle (nmf_amd/mesh.py:bake_textures; the reference exports
 * no textures).  Not on the training path.  Added without a bump of NMF_ABI_VERSION: no earlier prototype or workspace size changed.
 *
 * Layout.  The atlas is W x W texels, 4 <= W <= 16384, texel t = y W + x with row y = 0 the top row of the picture.  It is cut into
 * squares of T x T texels, n_sq = W / T (integer division) per row; square s = cy n_sq + cx holds face 2 s in its lower half and face
 * 2 s + 1 in its upper half.  T >= 4 and n_sq^2 >= ceil(F / 2) (nmf_amd.mesh.atlas_layout picks the largest such T).  With the local
 * texel (i, j) = (x - cx T, y - cy T) and b = T - 3: the lower face owns i + j <= T - 2 and has its corners 0, 1, 2 at (0, 0), (b, 0),
 * (0, b); the upper face owns the rest and is the same under i' = T - 1 - i, j' = T - 1 - j.  Owned texels outside the triangle (the
 * gutter a bilinear fetch inside the chart can reach) take the extrapolated barycentric point.  Unowned (face -1): squares past
 * ceil(F / 2), the upper half of the last square of an odd F, the W - n_sq T left-over rows and columns.
 *
 * nmf_atlas_texels: for the texels t0 .. t0 + n - 1, face_of [n] int32 (the owning face or -1) and pos [n][3] fp32, the world point
 *   of the texel on its face's plane; fp32, one rounding per operation, in this order (i, j: the local or the mirrored indices):
 *     b1 = i / b,  b2 = j / b,  b0 = (1 - b1) - b2,  p_c = (b0 v0_c + b1 v1_c) + b2 v2_c.
 *   verts [V][3] fp32, faces [F][3] int32.  Unowned texels get face -1 and position 0.  One launch, one lane per texel, closed form:
 *   no atomics, no search; two runs give the same bytes.  Refused (nothing launched): a null pointer (verts / faces may be NULL when
 *   F == 0), V or F below 0, W outside 4..16384, T below 4, above W or with (W / T)^2 < ceil(F / 2), n < 0, t0 < 0 or
 *   t0 + n > W^2 (NMF_EINVAL); n == 0 launches nothing.  A face index outside [0, V) is a caller error (NMF_ERANGE in the
 *   caller that can see the indices: they are device memory, so hip.atlas_texels reduces them once before the call); the kernel
 *   checks every index against V before it reads verts, and the texels of such a face come out unowned.
 *
 * nmf_atlas_store: one chunk of baked attributes -> the byte planes of the atlas.  face_of [n], albedo [n][3], f0 [n][3],
 *   roughness [n], normal [n][3] are indexed by t - t0; albedo_tex [W^2][3], f0_tex [W^2][3], rough_tex [W^2], normal_tex [W^2][3] by
 *   t.  Per value a NaN counts as 0 before anything else; the casts truncate:
 *     albedo     (uint8)(clamp(srgb(v), 0, 1) * 255), srgb(v) = v > 0.0031308 ? 1.055 pow(max(v, 0.0031308), 1 / 2.4) - 0.055 : 12.92 v
 *     f0, rough  (uint8)(clamp(v, 0, 1) * 255)
 *     normal     (uint8)clamp(v * 127 + 128, 0, 255)
 *   Unowned texels (face_of < 0) are 0 0 0 / 0 0 0 / 0 / 128 128 128 and their inputs are not read.  A null plane is skipped (its
 *   input may then be null too).  One launch; a lane owns the four texels of an aligned group and stores whole dwords where the group
 *   lies inside [t0, t0 + n) and the plane is 4-byte aligned, bytes otherwise: nothing outside [t0, t0 + n) of a plane is written.
 *   Refused (nothing launched): a null face_of, a plane without its input, W outside 4..16384, n < 0, t0 < 0 or t0 + n > W^2
 *   (NMF_EINVAL). */
int nmf_atlas_texels(const float* verts, const int32_t* faces, int64_t V, int64_t F, int32_t W, int32_t T, int64_t t0, int64_t n,
                     float* pos, int32_t* face_of, void* stream);
int nmf_atlas_store(const int32_t* face_of, const float* albedo, const float* f0, const float* roughness, const float* normal,
                    int64_t t0, int64_t n, int32_t W, uint8_t* albedo_tex, uint8_t* f0_tex, uint8_t* rough_tex, uint8_t* normal_tex,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Scene composition: several trained objects under one environment (nmf_amd/compose.py, csrc/compose.hip; the
 * reference's scripts/toaster_on_car.py over fields/listrf.py).  Not on the training path.  Added without a bump of
 * NMF_ABI_VERSION: no earlier prototype or workspace size changed.
 *
 * A placement maps an object's frame to the world: x_w = s R x_l + c, R [9] row-major rotation and c [3] HOST pointers, s > 0.
 *
 * nmf_rays_place: rays [B][6] = origin | direction between the two frames, one lane per ray; fp32, one rounding per operation:
 *     inverse = 1 (world -> local):  t = o - c,  o'_i = ((R_0i t_0 + R_1i t_1) + R_2i t_2) / s,  d'_i = (R_0i d_0 + R_1i d_1) + R_2i d_2
 *     inverse = 0 (local -> world):  o'_i = s ((R_i0 o_0 + R_i1 o_1) + R_i2 o_2) + c_i,          d'_i = (R_i0 d_0 + R_i1 d_1) + R_i2 d_2
 *   Directions are rotated only, never renormalised.  With R = I, c = 0, s = 1 exactly the rows are copied (the input's bits, a
 *   -0 included).  rays_out may be rays_in.  Refused (nothing launched): a null pointer (rays may be null when B == 0), B < 0, s or
 *   c not finite, s <= 0, inverse other than 0 / 1, max|R^T R - I| > 1e-4 (NMF_EINVAL).
 *
 * nmf_merge_rank: K lists of per-ray samples (CSR offsets [B+1] int64 over the same B rays, depths z [M_k] fp32 non-decreasing
 *   inside a ray, a positive scale each) -> the place dst_k [M_k] int64 of every sample in the merged list and its offsets
 *   offsets_m [B+1] = sum_k offsets_k.  The merged list of a ray is the stable K-way merge by world depth scale_k z: ascending
 *   depth, ties by list index, then by original order, i.e. the rank of a sample is its own index in its segment plus, per other
 *   list j, the number of entries with scale_j z_j < scale_k z, or equal and j < k (binary search).  One lane per sample, one
 *   launch, no atomics: two runs give the same bytes.  Lists with M_k == 0 and rays that are empty in every list are valid.  Every
 *   offset is clamped to [0, M_k] and every rank to its ray's merged segment before use.  Refused (nothing launched): K outside
 *   1..NMF_MERGE_MAX_LISTS (NMF_ERANGE); a null lists, offsets_m or offsets_k, a null z_k or dst_k where M_k > 0, M_k < 0, B < 0,
 *   samples with B == 0, a scale that is not finite and positive (NMF_EINVAL).
 *
 * nmf_merge_scatter: the rows of ONE list written to their places, one lane per sample; an output that is NULL is skipped (its
 *   input may then be NULL): sigma_m[d] = sigma[i] sigma_ratio, dist_m[d] = dist[i], z_m[d] = scale z[i],
 *   normal_m[d]_c = (R_c0 n_0 + R_c1 n_1) + R_c2 n_2, ray_id_m[d] = ray_id[i], part_m[d] = part, src_m[d] = i,
 *   inv_m[d] = inv[i] >= 0 ? inv[i] + row_base : -1, with d = dst[i]; a d outside [0, M_total) writes nothing.  The bounce-row map
 *   inv exists only after the list was shaded with the merged weights, so a caller scatters twice: the geometry before compositing,
 *   inv_m after shading.  Refused (nothing launched): M_k < 0, M_total < M_k, a null dst with M_k > 0, an output without its input,
 *   sigma_ratio or scale not finite and positive, normal_m with a null R or max|R^T R - I| > 1e-4 (NMF_EINVAL); part outside
 *   0..NMF_MERGE_MAX_LISTS - 1, M_k or row_base above 2^31 - 1 (NMF_ERANGE). */
#define NMF_MERGE_MAX_LISTS 8
typedef struct {
    const int64_t* offsets[NMF_MERGE_MAX_LISTS];   /* device [B+1] */
    const float* z[NMF_MERGE_MAX_LISTS];           /* device [M_k] */
    int64_t* dst[NMF_MERGE_MAX_LISTS];             /* device [M_k], written */
    float scale[NMF_MERGE_MAX_LISTS];
    int64_t M[NMF_MERGE_MAX_LISTS];
} nmf_merge_lists;
int nmf_rays_place(const float* rays_in, const float* R, const float* c, float s, int32_t inverse, int64_t B, float* rays_out,
                   void* stream);
int nmf_merge_rank(int32_t K, const nmf_merge_lists* lists, int64_t B, int64_t* offsets_m, void* stream);
int nmf_merge_scatter(int64_t M_k, int64_t M_total, const int64_t* dst, const float* sigma, const float* dist, const float* z,
                      const float* normal, const int32_t* ray_id, const int32_t* inv, float sigma_ratio, float scale, const float* R,
                      int32_t part, int64_t row_base, float* sigma_m, float* dist_m, float* z_m, float* normal_m, int32_t* ray_id_m,
                      int32_t* part_m, int32_t* src_m, int32_t* inv_m, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-sample frames: per-pixel accumulation of several passes and adaptive sample counts (nmf_amd/multisample.py:render_frame,
 * csrc/accum.hip; the reference renders one sample per pixel).  Not on the training path.  Added without a bump of
 * NMF_ABI_VERSION: no earlier prototype or workspace size changed.
 *
 * A frame has P = H W pixels, pixel p = row W + col.  A pixel list pix [n] is int32, strictly ascending; a NULL pix stands for all P
 * pixels in order (n is then not used; an empty list is a non-NULL pix with n = 0).  Per-pass arrays are indexed by the list entry i, the state and the finished maps by the
 * pixel.  Every kernel is one lane per pixel or list entry with plain loads and stores; every id read from a list is checked against
 * [0, P) before it indexes anything, and an entry outside is skipped.  Two runs give the same bytes.
 *
 * State.  nmf_accum_state_bytes(H, W) bytes (0 for a frame that would be refused), 4-byte aligned, allocated and ZEROED by the caller:
 * NMF_ACCUM_PLANES planes of P 4-byte words, plane k of pixel p at word k P + p --
 *     0 count (int32) | 1-3 mean rgb_lin | 4 mean acc | 5 mean depth | 6-8 mean normal | 9-11 mean rgb_map | 12-14 M2 of rgb_map
 * (fp32; M2 is the sum of squared deviations per channel), then one int32 per tile of NMF_ACCUM_TILE pixels, scratch of
 * nmf_accum_active.
 *
 * nmf_camera_rays_at: rays [n][6] (or [P][6] for a NULL list), row i the ray of pixel pix[i] through the point (col + ox, row + oy):
 *     x = ((col + ox) - cx) / fx,  y = ((row + oy) - cy) / fy, the rest as nmf_camera_rays, same order of operations.
 *   seed == 0: (ox, oy) = (jx, jy).  Otherwise a per-pixel rotation in [0, 1)^2 is added and wrapped, in uint32 arithmetic:
 *     mix(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
 *     h0 = mix(p 0x9E3779B1 + seed 0x85EBCA77),  h1 = mix(h0 + 0x9E3779B9),  u_k = (float)(h_k >> 8) 2^-24
 *     ox = jx + u_0; if (ox >= 1) ox = ox - 1;   oy likewise from jy and u_1            (fp32, one rounding per operation)
 *   jx = jy = 0.5, seed = 0 and a NULL list give the bytes of nmf_camera_rays.  Rows of skipped entries keep what they held.
 *   Refused (nothing launched): as nmf_camera_rays, and n < 0 or jx / jy outside [0, 1] (NMF_EINVAL), n above 2^31 - 1 (NMF_ERANGE);
 *   an empty list launches nothing.
 *
 * nmf_accum_update: folds one pass into the state for the pixels of the list.  rgb_lin [n][3], acc [n], rgb_map [n][3] (the
 *   displayed colour the pass formed), optionally depth [n] and normal [n][3] (NULL: those means are left alone).  Per pixel and
 *   value x (a NaN counts as 0), Welford's update, fp32, one rounding per operation:
 *     count += 1;  d = x - mean;  mean = mean + d / count;  and for rgb_map  M2 = M2 + d (x - mean).
 *   After one sample the means are the sample's bits.  A list that names a pixel twice is a caller error (the result is one of the
 *   two updates, nothing is written elsewhere).  Refused: H or W below 1, n < 0, a NULL state, rgb_lin, acc or rgb_map with n > 0,
 *   a misaligned state (NMF_EINVAL); H W or n above 2^31 - 1 (NMF_ERANGE).
 *
 * nmf_accum_active: list [<= P] = the ascending ids of the pixels that still need samples, *n_out (device int32) their number.  With
 *     se = max_c sqrt(M2_c / ((float)count (float)(count - 1)))  for count >= 2, else 0                  (display units)
 *   pixel p is active when count < min_spp, or count < max_spp and se > tol.  Three launches on the stream: the count of active pixels
 *   per tile, ONE workgroup that turns the tile counts into exclusive sums (and writes *n_out), and a second pass over the pixels
 *   that stores each active id at its tile's offset plus its rank inside the tile (ballots).  No atomics: the list is
 *   np.flatnonzero of the predicate.  Entries of list past *n_out are not written.  Refused: H or W below 1, min_spp < 0,
 *   max_spp < min_spp, tol negative or a NaN (+inf is allowed), a NULL or misaligned pointer (NMF_EINVAL); H W above 2^31 - 1
 *   (NMF_ERANGE).
 *
 * nmf_accum_resolve: the finished maps, each may be NULL: rgb_map [P][3] = (tonemap ? srgb(mean rgb_lin) : mean rgb_lin) +
 *   (1 - mean acc) bg with nmf_ray_compose_fwd's srgb and flags (the power taken in double and rounded to fp32 once); acc [P],
 *   depth [P], normal [P][3] the plain means (not renormalised: one sample gives the pass's own maps); se [P] as above; count [P] as
 *   float.  The average is taken on linear radiance and tonemapped afterwards; se is that of the displayed colour.  Refused: H or W
 *   below 1, a bg that is not finite, a NULL state, all six outputs NULL (NMF_EINVAL); H W above 2^31 - 1 (NMF_ERANGE). */
#define NMF_ACCUM_PLANES 15
#define NMF_ACCUM_TILE 256
int64_t nmf_accum_state_bytes(int32_t H, int32_t W);
int nmf_camera_rays_at(float r00, float r01, float r02, float r10, float r11, float r12, float r20, float r21, float r22, float tx,
                       float ty, float tz, float fx, float fy, float cx, float cy, int32_t H, int32_t W, float jx, float jy,
                       uint32_t seed, const int32_t* pix, int64_t n, float* rays, void* stream);
int nmf_accum_update(void* state, int32_t H, int32_t W, const int32_t* pix, int64_t n, const float* rgb_lin, const float* acc,
                     const float* rgb_map, const float* depth, const float* normal, void* stream);
int nmf_accum_active(void* state, int32_t H, int32_t W, int32_t min_spp, int32_t max_spp, float tol, int32_t* list, int32_t* n_out,
                     void* stream);
int nmf_accum_resolve(const void* state, int32_t H, int32_t W, float bg_r, float bg_g, float bg_b, int32_t tonemap, int32_t noclip,
                      float* rgb_map, float* acc, float* depth, float* normal, float* se, float* count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Denoised frames: a variance-guided, edge-stopping a-trous wavelet filter over the finished state of a multi-sample frame
 * (nmf_amd/multisample.py:FrameAccumulator.denoise, csrc/denoise.hip; spatial only -- SVGF without its temporal
 * part; the reference has no counterpart).  Not on the training path.  Added without a bump of NMF_ABI_VERSION: nothing existing
 * changed.
 *
 * Every quantity is fp32 with one rounding per operation, and the only operations are + - * / max fabs (sqrt once, for se), so the
 * kernels are restated bit for bit in numpy fp32.  One lane per pixel, plain loads and stores, no atomics: two runs give the same
 * bytes.  Pixel p = y W + x.  Read per pixel from the state of nmf_accum_* (its planes, above):
 *     L = mean rgb_lin [3] | A = mean acc | C = mean rgb_map [3], the guide colour in display units | Z = mean depth |
 *     N = mean normal [3], as stored | V = max_c (M2_c / ((float)n (float)(n - 1))) for a count n >= 2, else 0        (V = se^2)
 *
 * Workspace.  nmf_denoise_workspace_bytes(H, W) bytes (0 for a frame that would be refused), 4-byte aligned, need not be zeroed:
 * NMF_DENOISE_PLANES planes of P words, plane k of pixel p at word k P + p --
 *     0 fixed (int32) | 1 gx | 2 gy | 3-10 set 0: L [3], A, C [3], Vg | 11-18 set 1 likewise
 * N and Z are never filtered and are read from the state by every level.
 *
 * nmf_denoise_prepare (one launch): fixed = (V == 0); with indices clamped to the frame,
 *     r_j = (V[y+j][x-1] + 2 V[y+j][x]) + V[y+j][x+1]  for j = -1, 0, 1;   Vg = ((r_-1 + 2 r_0) + r_1) * 0.0625
 *     gx = (Z[y][x+1] - Z[y][x-1]) * 0.5;   gy = (Z[y+1][x] - Z[y-1][x]) * 0.5
 *   and L, A, C copied into set 0.
 *
 * nmf_denoise_level (one launch): reads set `src`, writes set 1 - src, with step s.  A fixed pixel copies its eight values bit for
 *   bit.  Otherwise the taps (i, j) run over {-2..2}^2, i outermost, q = (y + s i, x + s j); a tap outside the frame is skipped (both
 *   coordinates are checked before anything is read).  h = b_i b_j with b = (1, 4, 6, 4, 1) / 16 (exact).  The centre has w = h.
 *   Every other tap, with kc2 = k_c k_c, kn2 = k_n k_n, ka2 = k_a k_a (fp32 products taken on the host):
 *     d = ((dC_0^2 + dC_1^2) + dC_2^2) / (kc2 (Vg_p + Vg_q) + 1e-10)                      dC = C_p - C_q
 *     d = d + ((dN_0^2 + dN_1^2) + dN_2^2) / kn2                                          dN = N_p - N_q
 *     e = k_z fabs(gx_p (float)(s j) + gy_p (float)(s i)) + eps_z;   d = d + ((Z_p - Z_q) (Z_p - Z_q)) / (e e)
 *     d = d + ((A_p - A_q) (A_p - A_q)) / ka2
 *     t = max(0, 1 - d)  (0 for a NaN);   a tap with t = 0 is skipped;   w = (h t) t
 *   and in tap order  sw += w;  sL_c += w L_q;  sC_c += w C_q;  sA += w A_q;  sV += (w w) Vg_q.  Then
 *     L' = sL / sw,  C' = sC / sw,  A' = sA / sw,  Vg' = sV / (sw sw)                     (sw >= 36 / 256: the centre)
 *   A pixel to which no tap beside the centre contributed copies its eight values like a fixed one ((h x) / h need not return x).
 *   The kernel has compact support: nothing crosses an edge of depth, normal or coverage with d >= 1.  Vg' steers the colour test
 *   of the next level; it is a guide, not an estimate of the remaining error (the levels' inputs are correlated).
 *
 * nmf_denoise_finish (one launch) from set `src`, each output may be NULL: rgb_map [P][3] = (tonemap ? srgb(L) : L) + (1 - A) bg,
 *   the device function and flags of nmf_accum_resolve; rgb_lin [P][3] = L; acc [P] = A; se [P] = sqrt(Vg).  Straight after
 *   nmf_denoise_prepare (src = 0) rgb_map, rgb_lin and acc are nmf_accum_resolve's bytes.
 *
 * nmf_denoise: prepare, level l = 0 .. levels - 1 with s = 2^l and src = l & 1, finish with src = levels & 1, on the stream.
 *
 * Refused with nothing launched (NMF_EINVAL): H or W below 1; levels outside [0, NMF_DENOISE_MAX_LEVELS]; step outside
 * [1, 2^NMF_DENOISE_MAX_LEVELS]; src not 0 or 1; a k_* or eps_z that is not finite and positive; a bg that is not finite; a NULL or
 * misaligned state or workspace; all outputs NULL.  H W above 2^31 - 1: NMF_ERANGE. */
#define NMF_DENOISE_PLANES 19
#define NMF_DENOISE_MAX_LEVELS 8
int64_t nmf_denoise_workspace_bytes(int32_t H, int32_t W);
int nmf_denoise_prepare(const void* state, void* workspace, int32_t H, int32_t W, void* stream);
int nmf_denoise_level(const void* state, void* workspace, int32_t H, int32_t W, int32_t step, int32_t src, float k_c, float k_n,
                      float k_z, float eps_z, float k_a, void* stream);
int nmf_denoise_finish(const void* workspace, int32_t H, int32_t W, int32_t src, float bg_r, float bg_g, float bg_b, int32_t tonemap,
                       int32_t noclip, float* rgb_map, float* rgb_lin, float* acc, float* se, void* stream);
int nmf_denoise(const void* state, void* workspace, int32_t H, int32_t W, int32_t levels, float k_c, float k_n, float k_z, float eps_z,
                float k_a, float bg_r, float bg_g, float bg_b, int32_t tonemap, int32_t noclip, float* rgb_map, float* rgb_lin,
                float* acc, float* se, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NMF_HIP_H */
