// The training / evaluation pass of nmf_amd/fast_step.py (TrainPass.chunk / forward_autograd + backward_autograd / render_chunk) as
// ONE C++ call per chunk and direction: the C-ABI calls of a chunk in order, issued from C++ instead of from ~150 Python wrapper
// calls.  Included by host_ext.cpp (same namespace: it calls that file's wrappers directly).
//
// Why: in the regimes where a chunk has little device work (level 0 of every step, the early phase with 1000 re-traced rays,
// evaluation chunks, the 300^3 grid where the sample budget keeps ~2200 rays) the step was bound by the ~15 us of Python per
// launch (VERDICT round 2, item 3: "a C++ driver for one recursion level").  What stays in Python: everything per optimizer
// step (accumulators, end_step, Adam, controllers) and the per-step table rebuilds, which are queued BEFORE the call.
//
// Reference spans are the ones of fast_step.py: modules/tensor_nerf.py:210-674 (forward glue), models/microfacet.py:271-673
// (shading, re-trace selection), samplers/alphagrid.py:279-370 (sampler), train.py:598-708 (loss).
//
// The noise source and the replayed bookkeeping (noise.Pins) are Python objects called back through pybind: DeviceNoise
// answers from its pools in ~2 us, ReplayNoise / Pins (tests: the reference's fixtures run through THIS code) may be slow.
//
// A chunk OUTSIDE the pass (no bounce row, no secondary sample, maps without dense normals) throws UnsupportedChunk, which Python
// sees as nmf_amd.fast_step.Unsupported (host_ext.cpp: set_unsupported_class); every other error keeps its own type.

struct UnsupportedChunk : std::runtime_error { using std::runtime_error::runtime_error; };

struct RuntimeEvent {
    void* ev = nullptr;
    RuntimeEvent() {}
    void* get() {                       // created on first use (a StepCore may be constructed without a device)
        if (!ev) check(nmf_event_create(&ev), "nmf_event_create");
        return ev;
    }
    ~RuntimeEvent() { if (ev) nmf_event_destroy(ev); }
    RuntimeEvent(const RuntimeEvent&) = delete;
    RuntimeEvent& operator=(const RuntimeEvent&) = delete;
};

// two int64 sizes from the device to the host: the producing kernel PUBLISHES them into mapped, coherent host memory followed by a
// sequence number (the publish arguments of nmf_march_scan / nmf_bounce_index) and the host spins on that number (nmf_wait_seq) -- no copy
// command, no marker, no runtime signal wait.
struct SizeReadback {
    void* host = nullptr;
    void* dev = nullptr;
    int64_t seq = 0;
    ~SizeReadback() { if (host) nmf_host_free_mapped(host); }
    // -> (mapped device pointer, sequence number) to hand to the producing kernel
    std::pair<int64_t, int64_t> arm() {
        if (!host) check(nmf_host_alloc_mapped(&host, &dev, 64), "nmf_host_alloc_mapped");
        ++seq;
        return {reinterpret_cast<int64_t>(dev), seq};
    }
    static double& waited_us() { static double w = 0.0; return w; }      // host time spent waiting for sizes (tools/host_floor.py)
    static double* waited_by_slot() { static double w[4] = {0, 0, 0, 0}; return w; }     // ... by read-back of the chunk (0-3)
    static int& slot() { static int s = 0; return s; }
    std::pair<int64_t, int64_t> get() {
        struct Acc {
            std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
            ~Acc() {
                const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
                waited_us() += us;
                waited_by_slot()[slot() & 3] += us;
                ++slot();
            }
        } acc;
        py::gil_scoped_release nogil;
        check(nmf_wait_seq(host, seq, 30.0), "nmf_wait_seq");
        const int64_t* p = static_cast<const int64_t*>(host);
        return {p[0], p[1]};
    }
};

struct CoreSamples {
    Tensor xyzt, ray_id, step_id, dist, offsets, whole_valid, rays, valid;
    OT jitter, z;
    int64_t M = 0, b = 0, N = 0;
    // level 0 of a training chunk: the arrays are sized by the sample budget and (M, b) are still on the device (`live` = their
    // address) until the pipeline behind the sampler has been queued; live_rb then delivers them
    int64_t live = 0;
    SizeReadback* live_rb = nullptr;
};

struct CoreLevel {
    int lvl = 0;
    CoreSamples S;
    int64_t B = 0, M = 0, R = 0, Mb = 0;
    std::vector<int64_t> n_samples;
    Tensor offsets, sf, sg, w, conv, bidx, row_off, cnt32, inv, row_of_ray, j_of_ray, off, xyz_rows, app, heads;
    Tensor V, N, r1, f0, diff, feat, L, hl, dl, lpdf, mip, brays, incoming, bg, refl, rgb_map, acc, rgb_lin;
    OT gr, nr, brdf, brdf_mask, idx_re, idx_no, brays_re, mip_re, brays_no, mip_no, sf_rows, gr_rows, ori, rough;
    std::unique_ptr<CoreLevel> child;
    bool sparse_n = false, per_ray_bg = false;
};

class StepCore {
  public:
    // ---- configuration, set from Python (attributes; cheap to update per chunk) ----------------------------------------
    int64_t main_stream = 0;
    std::vector<int64_t> side_streams;              // raw handles: mlp0, mlp1, env0, env1, walk1, sat (0 entries: no overlap)
    py::object set_stream, main_stream_obj;         // torch.cuda.set_stream / the torch Stream objects: torch's CURRENT stream
    std::vector<py::object> side_stream_objs;       // follows a side block, so that the caching allocator ties what is allocated
                                                    // inside it (workspaces, outputs) to the stream that uses it
    bool overlap = true, sparse_normals = true;
    int64_t mlp_side_min_rays = 100000, mlp_side_min_env_rays = 200000, mlp_side_wgs_env = 256, walk_side_min_samples = 200000,
            mlp_side_wgs = 256, env_binned_from = 30000;
    // field
    int64_t vm_p = 0;
    std::vector<Tensor> dpk, dlk, apl, ali;         // fp32 tables: the backward walks (and the forward, unless f_* are set)
    std::vector<Tensor> f_dpk, f_dlk, f_apl, f_ali; // bf16-table variant: the copies the FORWARD queries read (empty: the fp32 ones)
    std::vector<Tensor> dpl, dli;                   // the density factors themselves [G,G,16] / [G,16]: value-only queries
    Tensor basis;
    // shading modules
    std::vector<double> head_p;
    Tensor head_W, head_b;
    std::vector<Tensor> mlp_ws;
    Tensor mlp_image;                   // nmf_brdf_mlp_pack of mlp_ws (undefined: the kernels convert the weights themselves)
    double mlp_bias = 0.0;
    Tensor sobol;
    // environment map
    Tensor env_table, env_pole, env_sc, env_act, env_bg, sh_conv;
    // sampler: parameter blocks (nmf_march_params) of the two levels, alpha bits
    int64_t march_p0 = 0, march_p1 = 0, max_samples = -1;
    OT alpha_bits, alpha_coarse;
    // model constants
    double scale = 25.0, anoise = 0.25, min_rough = 0.0, rays_per_ray = 128.0, test_rays_per_ray = 128.0;
    bool detach_n = false;
    std::vector<int64_t> max_brdf_rays, max_retrace_rays;
    Tensor white, one, select_ws;
    // accumulators of the optimizer step (views of TrainPass' flat buffer)
    std::vector<Tensor> g_dpk, g_dlk, g_apl, g_ali, g_mlp;
    Tensor g_basis, g_hW, g_hb, d_sat, d_pole, d_mip;
    OT d_bg_out;                                    // where the early env-map table backward writes (last chunk)
    // raw events recorded by the table rebuilds of this step on their side stream (0: the tables were built on the main stream)
    int64_t wait_tables = 0, wait_env = 0;
    bool used_env = false, early_env_done = false;
    bool env_split = true;                          // env adjoint of the bounce rays: d_dirs on the chain, the table role on a side stream
    int64_t env_split_min_lookups = 16384;
    bool env_keep_sat = false;                      // the early env-map table backward works on a copy of d_sat
    // data parallel: called from the LAST chunk's backward once the gradients of the shading modules and of the environment map are
    // final (everything but the field tables, which the walks that end the pass still write), with `comm_stream` waiting for
    // their producers -- the caller starts their all-reduce there, next to the walks (nmf_amd/trainer.py)
    py::object early_cb = py::none();
    int64_t comm_stream = 0;
    // The chunks of ONE optimizer step are independent given the parameters (train.py:509-712 runs them one after another): with
    // several chunk contexts (nmf_amd/fast_step.py: one StepCore + one set of streams each) chunk k + 1's forward is queued while chunk
    // k's backward runs.  `peer_streams` = the main streams of the OTHER contexts with work of this step in flight: what ends the
    // step here (the env-map table backward, the early all-reduce) also waits for what is queued on them.
    std::vector<int64_t> peer_streams;
    // ---- one training chunk, forward and backward apart ---------------------------------------------------------------------
    // train_forward keeps the level tree of the chunk until train_backward consumes it (ONE chunk may be pending: a second
    // forward drops the first).  This pair is what both callers run: chunk() below (nmf_amd.trainer.Trainer: loss head in between)
    // and the autograd node of TensorNeRF.forward(is_train=True) (nmf_amd/fast_step.py ChunkPass: the reference's own training loop,
    // train.py:509-747, calls forward, forms its loss with torch and calls backward()).
    // -> dict(kept, n_samples, [rgb_map, acc, ori, whole_valid, n_rays, n_rows]); n_samples == [0]: nothing to back-propagate
    py::dict train_forward(const Tensor& rays, double focal, py::object noise) {
        if (n_edits_ > 0) throw py::value_error("material edits are set: they are an evaluation feature and never enter a gradient "
                                                "(set_material_edits(None) before training)");
        pending_.reset();
        begin(noise);
        auto t = fwd(0, rays, focal, OT(), noise, true);
        py::dict out;
        out["kept"] = t->B;
        if (t->M == 0) {
            out["n_samples"] = std::vector<int64_t>{0};
            keep_.clear();
            return out;
        }
        out["n_samples"] = t->n_samples;
        {   // sizes of the chunk, for reports: secondary rays and bounce rows per level
            std::vector<int64_t> nr, nb;
            for (CoreLevel* l = t.get(); l; l = l->child.get()) { nr.push_back(l->R); nb.push_back(l->Mb); }
            out["n_rays"] = nr;
            out["n_rows"] = nb;
        }
        out["rgb_map"] = t->rgb_map;
        out["acc"] = t->acc;
        out["ori"] = *t->ori;
        out["whole_valid"] = t->S.whole_valid;
        pending_ = std::move(t);
        pending_keep_ = std::move(keep_);       // (an evaluation render between forward and backward must not release these)
        keep_.clear();
        return out;
    }
    bool has_pending() const { return (bool)pending_; }
    // d_acc / d_ori: adjoints of the per-ray accumulated opacity and orientation terms (None: zero).  last: every environment
    // adjoint of the optimizer step has been queued with this chunk -- the env-map table backward then starts on its side stream
    void train_backward(const Tensor& d_rgb, const OT& d_acc, const OT& d_ori, bool last) {
        if (!pending_) throw std::runtime_error("train_backward without a pending train_forward (the chunk was superseded by another forward)");
        std::unique_ptr<CoreLevel> t = std::move(pending_);
        keep_ = std::move(pending_keep_);
        pending_keep_.clear();
        dens_segs_.clear();
        app_segs_.clear();
        walk_forks_.clear();
        walk_clean_i_ = 0;
        last_chunk_ = last;
        bwd(*t, d_rgb.contiguous(), d_acc, d_ori);
        const bool early = last && comm_stream && !early_cb.is_none();
        if (early) {          // the communication stream starts where the main stream is NOW (and behind the env-map table backward) ...
            void* ev = next_ev();
            check(nmf_event_record(ev, st(main_stream)), "nmf_event_record");
            check(nmf_stream_wait_event(st(comm_stream), ev), "nmf_stream_wait_event");
            if (early_env_done && early_env_side_) {
                void* ev2 = next_ev();
                check(nmf_event_record(ev2, st(early_env_side_)), "nmf_event_record");
                check(nmf_stream_wait_event(st(comm_stream), ev2), "nmf_stream_wait_event");
            }
            for (int64_t ps : peer_streams)          // (the other chunk contexts' backwards write the same accumulators)
                if (ps != main_stream) side_waits_for(comm_stream, ps);
        }
        flush_walks();
        if (early) early_cb();      // ... and is fed once the walks have been queued: they are the critical path, the host work is not
    }

    // -> dict(loss (0-d tensor or None), total, kept, n_samples, rgb_map, acc, whole_valid)
    py::dict chunk(const Tensor& rays, const Tensor& gt, double focal, py::object noise, double inv_lbatch,
                   const std::vector<double>& wts, bool want_total, bool last, py::object l1_fn) {
        py::dict out = train_forward(rays, focal, noise);
        if (!pending_) {
            out["loss"] = py::none();
            return out;
        }
        CoreLevel* t = pending_.get();
        const int64_t b = t->rgb_map.size(0);
        Tensor gt_b = gt.narrow(0, 0, b).contiguous();
        // photometric term + the gradients of the loss mix (every term enters linearly with a constant weight, LossMix)
        Tensor loss, d_rgb, d_acc, d_ori;
        if (wts.size() == 4 && t->rgb_map.is_contiguous() && b == t->B) {
            if (!loss_ws_.defined() || loss_ws_.numel() < nmf_loss_head_workspace_bytes(b) || loss_ws_.device() != rays.device())
                loss_ws_ = at::zeros({std::max<int64_t>(2 * nmf_loss_head_workspace_bytes(b), 4096)}, rays.options().dtype(at::kByte));
            std::tie(loss, d_rgb, d_ori, d_acc) =          // wts = (photometric, L1, orientation, accumulated opacity)
                loss_head(t->rgb_map, gt_b, one, inv_lbatch, wts[0], wts[2], wts[3], loss_ws_, main_stream);
        } else {
            loss = sqerr_fwd(t->rgb_map, gt_b, main_stream);
            std::vector<std::vector<int64_t>> shapes = {{}, {}, {t->B}, {t->B}};
            std::vector<Tensor> dl = loss_mix_bwd(shapes, wts, inv_lbatch, one, main_stream);
            d_rgb = sqerr_bwd(t->rgb_map, gt_b, dl[0], main_stream);
            d_ori = dl[2]; d_acc = dl[3];
        }
        out["total"] = py::none();
        if (want_total) out["total"] = l1_fn(loss, *t->ori, t->acc);          // the chunk's total loss value (tests / traces)
        train_backward(d_rgb, d_acc, d_ori, last);
        out["loss"] = loss;
        return out;
    }

    // ---- one evaluation chunk (TrainPass.render_chunk) ------------------------------------------------------------------
    // want_maps: also the two per-ray maps of the reference's evaluation branch that need no dense appearance pass
    // (modules/tensor_nerf.py:480-501): depth = sum_k w_k z_k, world_normal = acc * sum_k w_k n_k + (1 - acc)
    // want_materials: also the material maps of level 0 (renderer.py:440-463) as one [B,15] block (nmf_material_maps: albedo |
    // roughness | diffuse | tint | spec).  Queued after the whole level tree: the appearance query over all kept
    // samples, then one launch; no noise is drawn and no launch the other outputs come from changes.
    // want_linear: also rgb_lin [B,3], the composited radiance sum_k w_k c_k before tonemap, clip and background: the buffer
    // nmf_ray_compose_fwd writes next to acc (nothing is launched or allocated for it)
    // -> dict(rgb_map, acc, kept, n_samples, [depth, world_normal], [materials], [rgb_lin]), or None when the sampler kept no sample
    py::object render(const Tensor& rays, double focal, py::object noise, bool want_maps, bool want_materials = false,
                      bool want_linear = false) {
        begin(noise);
        eval_z_ = want_maps;
        std::unique_ptr<CoreLevel> t;
        try {
            t = fwd(0, rays, focal, OT(), noise, false);
        } catch (...) {
            eval_z_ = false;
            throw;
        }
        eval_z_ = false;
        if (t->M == 0) return py::none();
        py::dict out;
        out["rgb_map"] = t->rgb_map;
        out["acc"] = t->acc;
        out["kept"] = t->B;
        out["n_samples"] = t->n_samples;
        if (want_materials) out["materials"] = material_maps_(*t);
        if (want_linear) out["rgb_lin"] = t->rgb_lin;
        if (want_maps) {
            if (!t->S.z.has_value() || !t->nr.has_value()) throw UnsupportedChunk("evaluation maps need the sampler's z values and dense normals");
            out["depth"] = segment_sum(t->S.z->view({t->M, 1}), OT(t->w), t->offsets, t->B, 1, main_stream).view({t->B});
            Tensor wn = segment_sum(*t->nr, OT(t->w), t->offsets, t->B, 1, main_stream);
            Tensor a = t->acc.unsqueeze(1);
            out["world_normal"] = a * wn + (1.0 - a);
        }
        return out;
    }

    // ---- material edits of the evaluation pass (nmf_heads_edit / nmf_material_maps_edit) ---------------------------------------
    // table: fp32 [K,32] (any device; a host copy is kept and checked by the C ABI at each use), or None / K = 0 for no edits.
    // Read only when !is_train: with edits every recursion level evaluates its heads in a launch of their own, edits them in place
    // and prepares the bounce rows from them (the unfused pair nmf_hip.h documents as bit-equal to nmf_bounce_prep_fwd_heads),
    // and the material maps take the _edit entry.  Without edits nothing changes: the same launches, the same bits.
    void set_material_edits(const OT& table) {
        if (!table.has_value() || !table->defined() || table->numel() == 0) {
            edits_ = Tensor();
            n_edits_ = 0;
            return;
        }
        if (table->dim() != 2 || table->size(1) != NMF_EDIT_ROW || table->scalar_type() != at::kFloat)
            throw py::value_error("set_material_edits: the table is fp32 [K,32]");
        if (table->size(0) > NMF_EDIT_MAX) throw py::value_error("set_material_edits: at most 16 edits");
        edits_ = table->detach().to(at::kCPU).contiguous().clone();
        n_edits_ = edits_.size(0);
    }
    int64_t n_material_edits() const { return n_edits_; }

  private:
    Tensor edits_;                 // host fp32 [K,32]
    int64_t n_edits_ = 0;
    // the material maps of level 0: appearance features of every kept sample (the forward query with appearance only), then
    // nmf_material_maps over the samples, their dense normals and the level's bounce rows
    Tensor material_maps_(CoreLevel& t) {
        if (!t.nr.has_value() || t.sparse_n || t.lvl != 0)
            throw UnsupportedChunk("material maps need the dense normals of level 0");
        if (!t.brdf.has_value() || !t.incoming.defined() || t.incoming.size(0) != t.R || !t.conv.defined() || !head_W.defined())
            throw UnsupportedChunk("material maps need the bounce rows' incoming radiance and BRDF weights");
        const int64_t M = t.M, B = t.B;
        Tensor xyzt = t.S.xyzt.narrow(0, 0, M).contiguous();
        Tensor app = *std::get<4>(vm_query_fwd(vm_p, xyzt, fw(f_dpk, dpk), fw(f_dlk, dlk), fw(f_apl, apl), fw(f_ali, ali), basis, false,
                                               false, true, false, main_stream));
        Tensor rays = t.S.rays.narrow(0, 0, B).contiguous();
        Tensor nr = t.nr->contiguous(), w = t.w.contiguous(), inv = t.inv.narrow(0, 0, M).contiguous();
        Tensor incoming = t.incoming.contiguous(), brdf = t.brdf->contiguous(), conv = t.conv.contiguous();
        Tensor maps = material_maps(app, nr, w, t.offsets.contiguous(), rays, head_W, head_b, head_p, conv, inv, t.row_off.contiguous(),
                                    t.cnt32.contiguous(), incoming, brdf, t.acc.contiguous(), t.bg.contiguous(), main_stream, OT(xyzt),
                                    n_edits_ > 0 ? OT(edits_) : OT());
        if (!trace_.is_none()) {       // tests: the inputs of the maps, for a restatement in float64
            trace_put("mm_app0", app); trace_put("mm_normals0", nr); trace_put("mm_w0", w); trace_put("mm_offsets0", t.offsets);
            trace_put("mm_rays0", rays); trace_put("mm_inv0", inv); trace_put("mm_row_off0", t.row_off); trace_put("mm_cnt0", t.cnt32);
            trace_put("mm_incoming0", incoming); trace_put("mm_brdf0", brdf); trace_put("mm_conv0", conv); trace_put("mm_acc0", t.acc);
            trace_put("mm_xyzt0", xyzt);
        }
        return maps;
    }

  public:
    bool env_table_backward_queued() const { return early_env_done; }
    bool env_was_used() const { return used_env; }
    void begin_step() { used_env = false; early_env_done = false; env_streams_.clear(); }

  private:
    py::object pins_, trace_;
    bool last_chunk_ = false;
    double near1_ = 0.0;
    SizeReadback rb_[8];
    int rb_next_ = 0;
    RuntimeEvent fork_ev_[16];
    int ev_next_ = 0;
    using Seg = std::tuple<Tensor, OT, OT, OT, OT, OT, OT>;
    std::vector<Seg> dens_segs_, app_segs_;
    std::vector<int64_t> walk_forks_;
    std::vector<Tensor> keep_;                       // tensors written / read on side streams: alive until the chunk ends

    std::unique_ptr<CoreLevel> pending_;             // train_forward's level tree, until train_backward takes it
    std::vector<Tensor> pending_keep_;

    // one walk over `segs` on `stream`.  The counters of the walk's brick sort live in a scratch kept from step to step: every walk
    // hands it back zero (the kernels that consume the counters clear them), so no memset launch precedes a sort.  One scratch per
    // walk of a chunk (walks of one chunk may overlap on their streams; chunks do not).  A walk that fails between the launches
    // that fill and clear the scratch would leave it non-zero: the scratch is dropped then, the next walk allocates a zeroed one.
    void walk_segments(std::vector<Seg>& segs, const OT& gb, int64_t stream) {
        // (R5: the brick sorts of the two walks that end the backward built as plans on an idle stream at the START of the backward --
        //  the walks then only permuted their adjoints -- took 108 us of kernels off the tail and gave them back in the
        //  saturated window before it: in-process A/B 1.328 -> 1.341 ms, removed.  R4 had the same result with the plans under the forward.)
        const auto* vp = reinterpret_cast<const nmf_vm_params*>(vm_p);
        const int64_t nb = nmf_vm_bwd_clean_bytes(vp->grid);
        if (walk_clean_i_ >= walk_clean_.size()) walk_clean_.emplace_back();
        Tensor& c = walk_clean_[walk_clean_i_++];
        if (!c.defined() || c.numel() != nb) c = at::zeros({nb}, std::get<0>(segs[0]).options().dtype(at::kByte));
        try {
            vm_query_bwd_segments(vm_p, segs, dpk, dlk, apl, ali, basis, g_dpk, g_dlk, g_apl, g_ali, gb, c, stream);
        } catch (...) {
            c = Tensor();
            throw;
        }
    }
    std::vector<Tensor> walk_clean_;
    size_t walk_clean_i_ = 0;
    SizeReadback& next_rb() { rb_next_ = (rb_next_ + 1) & 7; return rb_[rb_next_]; }
    void* next_ev() { ev_next_ = (ev_next_ + 1) & 15; return fork_ev_[ev_next_].get(); }

    void begin(py::object noise) {
        SizeReadback::slot() = 0;
        if (py::hasattr(noise, "begin_pass")) noise.attr("begin_pass")();
        pins_ = py::getattr(noise, "pins", py::none());
        trace_ = pins_.is_none() ? py::object(py::none()) : py::object(pins_.attr("trace"));
        dens_segs_.clear();
        app_segs_.clear();
        walk_forks_.clear();
        keep_.clear();
        walk_clean_i_ = 0;
        const auto* p1 = reinterpret_cast<const nmf_march_params*>(march_p1);
        near1_ = p1 ? p1->near_t : 0.0;
        need_tables_ = wait_tables != 0;
        need_env_ = wait_env != 0;
    }
    bool need_tables_ = false, need_env_ = false;
    bool eval_z_ = false;           // render(want_maps): the sampler also returns the z values of the kept samples
    OT mlp_img() const { return mlp_image.defined() ? OT(mlp_image) : OT(); }
    void tables_ready() {       // first read of the field tables / stacked weights in this chunk
        if (need_tables_) check(nmf_stream_wait_event(st(main_stream), reinterpret_cast<void*>(wait_tables)), "nmf_stream_wait_event");
        need_tables_ = false;
    }
    void env_ready() {          // first read of the env-map tables / SH irradiance in this chunk
        tables_ready();
        if (need_env_) check(nmf_stream_wait_event(st(main_stream), reinterpret_cast<void*>(wait_env)), "nmf_stream_wait_event");
        need_env_ = false;
    }

    static const std::vector<Tensor>& fw(const std::vector<Tensor>& f, const std::vector<Tensor>& m) { return f.size() == 3 ? f : m; }

    // side stream `which` waits for everything queued on the main stream so far and becomes torch's current stream until
    // end_side(); 0 when there is no overlap
    int64_t fork(int which) {
        if (!overlap || which >= (int)side_streams.size() || side_streams[which] == 0) return 0;
        void* ev = next_ev();
        check(nmf_event_record(ev, st(main_stream)), "nmf_event_record");
        check(nmf_stream_wait_event(st(side_streams[which]), ev), "nmf_stream_wait_event");
        set_stream(side_stream_objs[which]);
        return side_streams[which];
    }
    void end_side() { set_stream(main_stream_obj); }
    // the main stream waits for the side stream; tensors allocated under the side stream and consumed (and released) on the
    // main one are registered with the allocator
    void join(int64_t side, std::initializer_list<Tensor> made_on_side = {}) {
        void* ev = next_ev();
        check(nmf_event_record(ev, st(side)), "nmf_event_record");
        check(nmf_stream_wait_event(st(main_stream), ev), "nmf_stream_wait_event");
        if (made_on_side.size()) {
            const c10::Stream ms = c10::Stream::unpack3(main_stream_obj.attr("stream_id").cast<int64_t>(),
                                                        main_stream_obj.attr("device_index").cast<c10::DeviceIndex>(),
                                                        static_cast<c10::DeviceType>(main_stream_obj.attr("device_type").cast<int>()));
            for (const Tensor& x : made_on_side)
                if (x.defined()) x.record_stream(ms);
        }
    }

    Tensor env_fwd(const Tensor& rows, const Tensor& sa) {
        env_ready();
        return sat_lookup_fwd(env_table, rows, sa, 0.0, env_pole, env_sc, main_stream);
    }
    // side stream `side` also waits for what side stream `other` has queued
    void side_waits_for(int64_t side, int64_t other) {
        void* ev = next_ev();
        check(nmf_event_record(ev, st(other)), "nmf_event_record");
        check(nmf_stream_wait_event(st(side), ev), "nmf_stream_wait_event");
    }
    std::vector<int64_t> env_streams_;          // side streams with env-map adjoints of this optimizer step in flight
    void env_stream_used(int64_t s) {
        if (s && std::find(env_streams_.begin(), env_streams_.end(), s) == env_streams_.end()) env_streams_.push_back(s);
    }
    Tensor env_bwd(const Tensor& rows, const Tensor& sa, const Tensor& d_out, int64_t stream) {
        used_env = true;
        const int64_t R = rows.size(0);
        if (env_split && overlap && stream == main_stream && R >= env_binned_from && R >= env_split_min_lookups && d_out.is_contiguous()) {
            // the backward chain (the sampler's adjoint) needs d_dirs only: the dual-number role alone on the chain, the table role
            // (count / records / accumulate: d_sat, needed at the end of the step) on a stream of its own
            Tensor dd = sat_lookup_bwd_dirs(env_table, rows, sa, 0.0, d_out, d_pole, d_mip, env_sc, main_stream);
            const int64_t ts = fork(6);
            if (ts) {
                sat_lookup_bwd_table(env_table, rows, sa, 0.0, d_out, d_sat, env_sc, ts);
                end_side();
                env_stream_used(ts);
                walk_forks_.push_back(ts);          // joined with the walks at the end of the chunk's backward
                keep_.push_back(rows); keep_.push_back(sa); keep_.push_back(d_out);
            } else {
                sat_lookup_bwd_table(env_table, rows, sa, 0.0, d_out, d_sat, env_sc, main_stream);
            }
            return dd;
        }
        if (stream != main_stream) env_stream_used(stream);
        OT dd = sat_lookup_bwd(env_table, rows, sa, 0.0, d_out, d_sat, d_pole, d_mip, true, env_sc, env_binned_from, stream);
        return *dd;
    }

    Tensor uniform(py::object& noise, std::vector<int64_t> shape) { return noise.attr("uniform")(py::tuple(py::cast(shape))).cast<Tensor>(); }
    void skip(py::object& noise, const char* kind, std::vector<int64_t> shape) { noise.attr("skip")(kind, py::tuple(py::cast(shape))); }
    void trace_put(const std::string& key, const Tensor& t) {
        if (trace_.is_none()) return;
        py::dict d = trace_.cast<py::dict>();
        d[py::str(key)] = py::cast(t);
    }

    // ---- sampler (AlphaGridSampler.sample_begin / sample_finish) ------------------------------------------------------
    struct Pending { SizeReadback* rb; nmf_march_params p; Tensor rays, valid, offsets, wv, totals; OT jitter; int64_t N; py::object py_pending; };

    Pending sample_begin(int lvl, const Tensor& rays_in, py::object& noise, bool is_train, py::object& sampler, double focal) {
        Pending P;
        if (!pins_.is_none()) {       // replayed occupancy decisions: the Python sampler (tests)
            P.py_pending = sampler.attr("sample_begin")(rays_in, focal, lvl == 0 ? py::object(py::none()) : py::object(py::float_(near1_)),
                                                        is_train, lvl == 0, noise);
            P.rb = nullptr;
            return P;
        }
        P.p = *reinterpret_cast<const nmf_march_params*>(lvl == 0 ? march_p0 : march_p1);
        P.N = P.p.n_steps;
        P.rays = rays_in.contiguous();
        if (is_train) {
            py::tuple j = noise.attr("jitter")(P.rays.size(0), P.N).cast<py::tuple>();
            if (!j[0].is_none()) P.jitter = j[0].cast<Tensor>();
            py::tuple so = j[1].cast<py::tuple>();
            P.p.seed = so[0].cast<uint64_t>();
            P.p.offset = so[1].cast<uint64_t>();
        }
        P.p.is_train = is_train ? 1 : 0;
        Tensor counts;
        std::tie(P.valid, counts) = march_count(reinterpret_cast<int64_t>(&P.p), P.rays, P.jitter, alpha_bits, alpha_coarse, main_stream);
        const int64_t budget = (max_samples > 0 && is_train && lvl == 0) ? max_samples : -1;
        Tensor totals;
        P.rb = &next_rb();
        const auto pub = P.rb->arm();
        std::tie(P.offsets, P.wv, totals) = march_scan(counts, budget, main_stream, pub.first, pub.second);
        P.totals = totals;
        keep_.push_back(totals);
        return P;
    }

    // live: do not wait for (M, b); fill at the capacity the sample budget guarantees (alphagrid.py:353-364: the kept total stays
    // below max_samples) -- the rays past b have empty sample ranges (nmf_march_scan clamps their offsets), so the fill and the
    // composite may run over all rays; the queries behind them read the count from the device
    CoreSamples sample_finish(Pending& P, py::object& sampler, bool live = false) {
        CoreSamples S;
        if (P.rb == nullptr) {
            py::object s = sampler.attr("sample_finish")(P.py_pending);
            S.xyzt = s.attr("xyzt").cast<Tensor>(); S.ray_id = s.attr("ray_id").cast<Tensor>(); S.step_id = s.attr("step_id").cast<Tensor>();
            S.dist = s.attr("dist").cast<Tensor>(); S.offsets = s.attr("offsets").cast<Tensor>();
            S.whole_valid = s.attr("whole_valid").cast<Tensor>(); S.rays = s.attr("rays").cast<Tensor>();
            if (eval_z_ && py::hasattr(s, "z") && !s.attr("z").is_none()) S.z = s.attr("z").cast<Tensor>();
            S.M = s.attr("M").cast<int64_t>(); S.b = s.attr("b").cast<int64_t>(); S.N = s.attr("N").cast<int64_t>();
            return S;
        }
        int64_t M, b;
        if (live) {
            b = P.rays.size(0);
            M = std::min<int64_t>(max_samples, b * P.N);
            S.live = reinterpret_cast<int64_t>(P.totals.data_ptr());
            S.live_rb = P.rb;
        } else {
            std::tie(M, b) = P.rb->get();
        }
        std::tie(S.xyzt, S.ray_id, S.step_id, S.z, S.dist) =
            march_fill(reinterpret_cast<int64_t>(&P.p), P.rays, b, M, P.jitter, P.valid, P.offsets, !live && eval_z_, main_stream);
        S.offsets = P.offsets; S.whole_valid = P.wv.view(at::kBool); S.rays = P.rays; S.valid = P.valid; S.jitter = P.jitter;
        S.M = M; S.b = b; S.N = P.N;
        return S;
    }

  public:
    py::object sampler;      // AlphaGridSampler (only called when bookkeeping is replayed)

  private:
    // ---- forward of one recursion level -------------------------------------------------------------------------------
    std::unique_ptr<CoreLevel> fwd(int lvl, const Tensor& rays, double focal, const OT& start_mip, py::object& noise, bool is_train,
                                   const std::function<void()>& filler = nullptr) {
        auto t = std::make_unique<CoreLevel>();
        t->lvl = lvl;
        Pending P = sample_begin(lvl, rays, noise, is_train, sampler, focal);
        if (filler) filler();
        // level 0 of a training chunk: everything up to the bounce index is queued behind the sampler's scan without waiting for
        // its sizes (the first of the chunk's four read-backs goes away: the host used to issue these six launches one by one
        // into an empty queue, 120 us for 57 us of kernels)
        const bool live = lvl == 0 && is_train && P.rb != nullptr && max_samples > 0 && !filler && pins_.is_none() &&
                          py::hasattr(noise, "capacity_draws");
        t->S = sample_finish(P, sampler, live);
        CoreSamples& S = t->S;
        int64_t B = S.b, M = S.M;
        t->B = B; t->M = M;
        t->n_samples = {M};
        if (M == 0) {
            env_ready();          // the caller falls back to the module path on the main stream: the rebuilt tables must be behind it
            return t;
        }
        t->offsets = S.offsets.narrow(0, 0, B + 1);
        const bool sparse_n = lvl > 0 && sparse_normals;
        t->sparse_n = sparse_n;
        tables_ready();
        if (sparse_n && dpl.size() == 3) {
            Tensor sf, sg;
            std::tie(sf, sg) = vm_query_sigma(vm_p, S.xyzt, dpl, dli, main_stream);
            t->sf = sf; t->sg = sg;
        } else {
            auto q = vm_query_fwd(vm_p, S.xyzt, fw(f_dpk, dpk), fw(f_dlk, dlk), fw(f_apl, apl), fw(f_ali, ali), basis, true, !sparse_n, false,
                                  false, main_stream, S.live);
            t->sf = *std::get<0>(q); t->sg = *std::get<1>(q); t->gr = std::get<2>(q); t->nr = std::get<3>(q);
        }
        Tensor acc0;
        std::tie(t->w, acc0) = composite_fwd(t->sg, S.dist, t->offsets, B, scale, main_stream);
        // ---- Microfacet.shade_compact, sparse appearance (same draw order as the autograd path)
        py::object deferred = noise.attr("normal_deferred")(py::make_tuple(M, 24));
        skip(noise, "randn", {M, 3});
        skip(noise, "randn", {M, 2});
        skip(noise, "rand", {5000});
        skip(noise, "rand", {5000});
        // the bounce counts: computed inside the two launches of the bounce index (nmf_bounce_index_select; replayed
        // bookkeeping: a launch of their own first)
        Tensor counts, sel_u;
        OT sel_total;
        int64_t sel_mode = 0;
        double sel_mul = 0.0, sel_add = 0.0;
        if (lvl == 0) {
            sel_u = uniform(noise, {M}).contiguous();
            sel_mode = 0; sel_mul = is_train ? rays_per_ray : test_rays_per_ray; sel_add = 0.0;
        } else {
            Tensor total;
            if (py::hasattr(noise, "select_dense_parts")) {
                py::tuple r = noise.attr("select_dense_parts")(S.b, S.N, M).cast<py::tuple>();
                sel_u = r[0].cast<Tensor>().contiguous();
                total = select_total(t->w, sel_u, r[1].cast<double>(), select_ws, main_stream);
            } else {
                py::tuple r = noise.attr("select_dense")(S.b, S.N, S.ray_id, S.step_id).cast<py::tuple>();
                sel_u = r[0].cast<Tensor>().contiguous();
                total = (t->w.sum(at::kDouble) + 1e-3 * r[1].cast<Tensor>()).to(at::kFloat).clamp_min(1e-3);
            }
            const int64_t nb = max_brdf_rays.at(lvl) - M;
            sel_mode = 1;
            if (nb > 0) { sel_mul = (double)nb; sel_add = 1.0; }
            else { sel_mul = (double)max_brdf_rays.at(lvl); sel_add = 0.5; }
            sel_total = total;
            keep_.push_back(total);
        }
        const bool fused_select = pins_.is_none() && M <= (int64_t(1) << 20);
        if (!fused_select) {
            counts = select_bounces(t->w, sel_u, sel_mode, sel_mul, sel_add, 1.0, sel_total, main_stream);
            if (!pins_.is_none()) counts = pins_.attr("counts_for")(lvl, counts).cast<Tensor>();
        }
        Tensor tot, xyz_rows;
        SizeReadback& rb = next_rb();
        {
            const auto pub = rb.arm();
            py::tuple r = fused_select ? bounce_index_select(t->w, sel_u, sel_mode, sel_mul, sel_add, 1.0, sel_total, S.xyzt, main_stream,
                                                             pub.first, pub.second, S.live)
                                       : bounce_index(counts, S.xyzt, main_stream, pub.first, pub.second, S.live);
            t->bidx = r[0].cast<Tensor>(); t->row_off = r[1].cast<Tensor>(); t->cnt32 = r[2].cast<Tensor>();
            t->inv = r[3].cast<Tensor>(); tot = r[4].cast<Tensor>(); xyz_rows = r[5].cast<Tensor>();
            keep_.push_back(tot);
            keep_.push_back(sel_u);
        }
        t->conv = sh_conv;
        const bool per_ray_bg = lvl > 0;
        t->per_ray_bg = per_ray_bg;
        if (per_ray_bg) {
            t->rough = start_mip->narrow(0, 0, B).contiguous();
            t->bg = env_fwd(B == S.rays.size(0) ? S.rays : S.rays.narrow(0, 0, B), *t->rough);
        } else {
            t->bg = white;
        }
        auto [R, Mb] = rb.get();
        if (S.live) {               // the sizes of the sampler (published long before the bounce index's): shrink the capacity-sized arrays
            auto [Ml, bl] = S.live_rb->get();
            S.live = 0;
            M = Ml; B = bl;
            S.M = Ml; S.b = bl; t->M = Ml; t->B = bl;
            t->n_samples = {Ml};
            if (Ml == 0) {
                env_ready();
                return t;
            }
            S.xyzt = S.xyzt.narrow(0, 0, Ml); S.ray_id = S.ray_id.narrow(0, 0, Ml); S.step_id = S.step_id.narrow(0, 0, Ml);
            S.dist = S.dist.narrow(0, 0, Ml);
            t->offsets = S.offsets.narrow(0, 0, bl + 1);
            t->sf = t->sf.narrow(0, 0, Ml); t->sg = t->sg.narrow(0, 0, Ml); t->w = t->w.narrow(0, 0, Ml);
            if (t->gr.has_value()) t->gr = t->gr->narrow(0, 0, Ml);
            if (t->nr.has_value()) t->nr = t->nr->narrow(0, 0, Ml);
            t->inv = t->inv.narrow(0, 0, Ml);
        }
        if (R == 0) {
            env_ready();
            throw UnsupportedChunk("no bounce rows");
        }
        t->R = R; t->Mb = Mb;
        t->bidx = t->bidx.narrow(0, 0, Mb); t->row_off = t->row_off.narrow(0, 0, Mb + 1); t->cnt32 = t->cnt32.narrow(0, 0, Mb);
        std::tie(t->row_of_ray, t->j_of_ray) = expand_segments(t->row_off, Mb, R, main_stream);
        t->off = uniform(noise, {Mb, 1, 2}).reshape({Mb, 2}).contiguous();
        t->xyz_rows = xyz_rows.narrow(0, 0, Mb);
        OT feat_noise;
        {
            py::object fn = noise.attr("rows")(deferred, t->bidx);
            if (!fn.is_none()) feat_noise = fn.cast<Tensor>();
        }
        if (sparse_n) {
            Tensor sfr, grr, nrr;
            std::tie(sfr, grr, nrr) = vm_query_rows(vm_p, t->xyz_rows, fw(f_dpk, dpk), fw(f_dlk, dlk), main_stream);
            t->sf_rows = sfr; t->gr_rows = grr; t->nr = nrr;
        }
        t->app = *std::get<4>(vm_query_fwd(vm_p, t->xyz_rows, fw(f_dpk, dpk), fw(f_dlk, dlk), fw(f_apl, apl), fw(f_ali, ali), basis, false,
                                           false, true, false, main_stream));
        Tensor xyz;
        env_ready();                 // the material heads are evaluated inside the row preparation (one launch per level)
        if (!is_train && n_edits_ > 0) {   // material edits: heads, edit in place, row preparation from the edited heads
            t->heads = heads_fwd(t->app, head_W, head_b, head_p, main_stream);
            heads_edit(t->heads, t->xyz_rows, edits_, main_stream);
            std::tie(t->V, t->N, t->r1, t->f0, t->diff, t->feat, xyz) =
                bounce_prep_fwd(t->bidx, *t->nr, t->app, t->heads, S.xyzt, S.ray_id, S.rays, t->conv, feat_noise, anoise, -1e30,
                                sparse_n ? 2 : 1, main_stream);
        } else {
            std::tie(t->heads, t->V, t->N, t->r1, t->f0, t->diff, t->feat, xyz) =
                bounce_prep_fwd_heads(t->bidx, *t->nr, t->app, head_W, head_b, head_p, S.xyzt, S.ray_id, S.rays, t->conv, feat_noise,
                                      anoise, is_train ? min_rough : -1e30, sparse_n ? 2 : 1, main_stream);
        }
        std::tie(t->L, t->hl, t->dl, t->lpdf, t->mip, t->brays) =
            ggx_rays_fwd(t->V, t->N, t->r1, xyz, t->off, t->cnt32, sobol, t->row_of_ray, t->j_of_ray, main_stream);
        const bool has_retrace = lvl < (int)max_retrace_rays.size();
        const bool sorts = !pins_.is_none() && pins_.attr("sorts")(lvl).cast<bool>();
        const int64_t num_retrace = has_retrace ? std::min<int64_t>(R, max_retrace_rays[lvl]) : 0;
        const bool full_retrace = has_retrace && num_retrace >= R && !sorts;
        auto mlp = [&]() {
            Tensor o, mk;
            std::tie(o, mk) = brdf_mlp_fwd(mlp_ws, t->hl, t->dl, t->feat, t->r1, t->row_of_ray, mlp_bias, is_train, 0, main_stream, mlp_img());
            t->brdf = o;
            if (is_train) t->brdf_mask = mk;
        };
        if (!full_retrace) mlp();
        // ---- incoming radiance of the secondary rays (models/microfacet.py:475-563)
        if (has_retrace) {
            if (full_retrace) {
                skip(noise, "rand", {R});
                t->child = fwd(lvl + 1, t->brays, focal, t->mip, noise, is_train, mlp);     // the MLP runs under the child's read-back
                if (t->child->M == 0) throw UnsupportedChunk("no secondary sample");
                t->n_samples.insert(t->n_samples.end(), t->child->n_samples.begin(), t->child->n_samples.end());
                t->incoming = t->child->rgb_map;
            } else {
                Tensor w_rows = at::index_select(t->w, 0, t->bidx);
                Tensor cc = retrace_scores_(*t->brdf, t->V, t->N, t->lpdf, w_rows, t->cnt32, t->row_of_ray);
                cc = cc / cc.sum() * (double)num_retrace;
                cc = cc + uniform(noise, {R});
                const int64_t cut = std::max<int64_t>(R - num_retrace, 0);
                if (pins_.is_none()) {
                    // the reference only uses its argsort as a partition (microfacet.py:506-537): radix select, the selected
                    // rays in argsort order (they are marched in it), the others in index order
                    Tensor top, rest;
                    std::tie(top, rest) = topk_select_(cc.contiguous(), R - cut);
                    t->idx_re = top.to(at::kLong);
                    t->idx_no = rest.to(at::kLong);
                } else {
                    Tensor order = argsort_(cc.contiguous()).to(at::kLong);
                    trace_put("retrace_order_own" + std::to_string(lvl), order);
                    py::dict ro = pins_.attr("retrace_order").cast<py::dict>();
                    if (ro.contains(py::int_(lvl))) order = ro[py::int_(lvl)].cast<Tensor>().to(order.device());
                    t->idx_re = order.narrow(0, cut, R - cut);
                    t->idx_no = order.narrow(0, 0, cut);
                    trace_put("retrace_score" + std::to_string(lvl), cc);
                    trace_put("retrace_order" + std::to_string(lvl), order);
                    trace_put("retrace_idx" + std::to_string(lvl), *t->idx_re);
                }
                t->incoming = at::empty({R, 3}, rays.options().dtype(at::kFloat));
                if (t->idx_re->size(0) > 0) {
                    t->brays_re = at::index_select(t->brays, 0, *t->idx_re);
                    t->mip_re = at::index_select(t->mip, 0, *t->idx_re);
                    t->child = fwd(lvl + 1, *t->brays_re, focal, t->mip_re, noise, is_train);
                    if (t->child->M == 0) throw UnsupportedChunk("no secondary sample");
                    t->n_samples.insert(t->n_samples.end(), t->child->n_samples.begin(), t->child->n_samples.end());
                    t->incoming.index_copy_(0, *t->idx_re, t->child->rgb_map);
                }
                if (t->idx_no->size(0) > 0) {
                    t->brays_no = at::index_select(t->brays, 0, *t->idx_no);
                    t->mip_no = at::index_select(t->mip, 0, *t->idx_no);
                    skip(noise, "rand", {t->idx_no->size(0)});
                    skip(noise, "rand", {t->idx_no->size(0)});
                    t->incoming.index_copy_(0, *t->idx_no, env_fwd(*t->brays_no, *t->mip_no));
                }
            }
        } else {
            skip(noise, "rand", {R});
            skip(noise, "rand", {R});
            t->incoming = env_fwd(t->brays, t->mip);
        }
        // ---- Fresnel mix + per-ray sums, tonemap, background
        if (per_ray_bg) {
            skip(noise, "rand", {B});
            skip(noise, "rand", {B});
        }
        Tensor contrib = shade_mix_fwd(t->V, t->f0, t->diff, t->cnt32, t->row_of_ray, t->L, t->incoming, *t->brdf, main_stream);
        t->refl = segment_sum(contrib, OT(), t->row_off, Mb, 8, main_stream);
        std::tie(t->rgb_map, t->acc, t->rgb_lin, t->ori) =
            ray_compose_fwd(t->w, t->refl, t->inv, lvl == 0 ? t->nr : OT(), S.rays, t->offsets, B, t->bg, per_ray_bg, lvl == 0, false,
                            lvl == 0, main_stream);
        if (!trace_.is_none()) {
            const std::string s = std::to_string(lvl);
            trace_put("rgb_map" + s, t->rgb_map); trace_put("acc_map" + s, t->acc); trace_put("whole_valid" + s, S.whole_valid);
            trace_put("incoming" + s, t->incoming);
            if (t->ori.has_value()) trace_put("ori" + s, *t->ori);
        }
        return t;
    }

    // retrace scores / argsort live in retrace.hip; thin local wrappers (no C++ twin existed: the early phase only)
    Tensor retrace_scores_(const Tensor& brdf, const Tensor& V, const Tensor& N, const Tensor& lpdf, const Tensor& w_rows,
                           const Tensor& cnt, const Tensor& row_of_ray) {
        const int64_t R = row_of_ray.size(0);
        Tensor o = fe(V, {R});
        check(nmf_retrace_scores(f32(brdf), f32(V), f32(N), f32(lpdf), f32(w_rows), i32(cnt), i32(row_of_ray), R, out(o), st(main_stream)),
              "nmf_retrace_scores");
        return o;
    }
    std::pair<Tensor, Tensor> topk_select_(const Tensor& keys, int64_t k) {
        const int64_t n = keys.size(0);
        Tensor top = ie(keys, {k}, at::kInt), rest = ie(keys, {n - k}, at::kInt);
        const int64_t nbytes = nmf_topk_select_workspace_bytes(n);
        Tensor ws = ie(keys, {(nbytes + 7) / 8}, at::kLong);
        check(nmf_topk_select(f32(keys), n, k, k ? static_cast<int32_t*>(top.data_ptr()) : nullptr,
                              n - k ? static_cast<int32_t*>(rest.data_ptr()) : nullptr, ws.data_ptr(), nbytes, st(main_stream)),
              "nmf_topk_select");
        return {top, rest};
    }
    Tensor argsort_(const Tensor& keys) {
        const int64_t n = keys.size(0);
        Tensor idx = ie(keys, {n}, at::kInt);
        const int64_t nbytes = nmf_argsort_workspace_bytes(n);
        Tensor ws = ie(keys, {(nbytes + 7) / 8}, at::kLong);
        check(nmf_argsort_f32(f32(keys), n, static_cast<int32_t*>(idx.data_ptr()), ws.data_ptr(), nbytes, st(main_stream)),
              "nmf_argsort_f32");
        return idx;
    }

    // ---- backward of one recursion level ------------------------------------------------------------------------------
    // -> adjoint of the level's rays [B,6] (undefined tensor at level 0)
    Tensor bwd(CoreLevel& t, const Tensor& d_rgb, const OT& d_acc, const OT& d_ori) {
        CoreSamples& S = t.S;
        const int lvl = t.lvl;
        const bool view = lvl > 0;
        Tensor d_w;
        OT d_refl, d_nrm;
        std::tie(d_w, d_refl, d_nrm) =
            ray_compose_bwd(t.w, t.refl, t.inv, d_ori.has_value() ? t.nr : OT(), S.rays, S.ray_id, t.bg, t.per_ray_bg, lvl == 0, false,
                            t.rgb_lin, d_rgb, d_acc, d_ori, d_ori.has_value(), main_stream);
        // the value-only walk of a level with sparse normals goes to a side stream from here, next to everything below it.  (Measured and
        // removed in round 4: the walk queued after the levels below, 1.627 vs 1.577 ms; the composite backward at the head of that
        // side stream, neutral.)
        Tensor d_sigma = composite_bwd(t.sg, S.dist, t.w, t.offsets, t.B, scale, d_w, main_stream);
        bool early_walk = false;
        if (t.sparse_n && t.M >= walk_side_min_samples) {
            const int64_t ws = fork(4);
            if (ws) {
                std::vector<Seg> segs = {Seg(S.xyzt, t.sf, OT(), d_sigma, OT(), OT(), OT())};
                walk_segments(segs, OT(), ws);
                end_side();
                walk_forks_.push_back(ws);
                keep_.push_back(d_sigma);
                keep_.push_back(d_w);
                early_walk = true;
            }
        }
        Tensor d_rays;
        int64_t env_side = 0;
        if (t.per_ray_bg) {
            Tensor d_bg = bg_adjoint(t.acc, d_rgb, main_stream);
            Tensor env_rows = t.B == S.rays.size(0) ? S.rays : S.rays.narrow(0, 0, t.B);
            env_side = t.B >= mlp_side_min_rays ? fork(2 + (lvl > 0 ? 1 : 0)) : 0;
            d_rays = env_bwd(env_rows, *t.rough, d_bg, env_side ? env_side : main_stream);
            if (env_side) end_side();
            keep_.push_back(d_bg);
        }
        Tensor d_inc, d_brdf, dL, d_fd, dV, dV_rows;
        if (view) {
            std::tie(d_inc, d_brdf, dL, d_fd, dV) =
                shade_mix_bwd_view(t.V, t.f0, t.diff, t.cnt32, t.row_of_ray, t.L, t.incoming, *t.brdf, *d_refl, main_stream);
            dV_rows = segment_sum(dV, OT(), t.row_off, t.Mb, 8, main_stream);
        } else {
            std::tie(d_inc, d_brdf, dL, d_fd) =
                shade_mix_bwd(t.V, t.f0, t.diff, t.cnt32, t.row_of_ray, t.L, t.incoming, *t.brdf, *d_refl, main_stream);
        }
        Tensor rows6 = segment_sum_wide(d_fd, 6, t.row_off, t.Mb, main_stream);
        // ---- BRDF MLP backward: on a side stream next to the adjoint of the bounce rays below
        const int64_t n_re = t.idx_re.has_value() ? t.idx_re->size(0) : (t.child ? t.R : 0);
        const int64_t n_env = t.R - n_re;
        const bool below = t.child && t.child->B >= mlp_side_min_rays;
        // (Measured and removed in round 4: ONE launch for this level's rays and the level below's, nmf_brdf_mlp_bwd_segments, 1.383 ->
        // 1.486 ms -- the merged launch starts later, into a chip the value walk and the env adjoint already fill.)
        Tensor d_feat;
        bool have_feat = false;
        const int64_t mlp_side = (below || n_env >= mlp_side_min_env_rays) ? fork(lvl > 0 ? 1 : 0) : 0;
        if (mlp_side) {
            d_feat = brdf_mlp_bwd(mlp_ws, t.hl, t.dl, t.feat, t.r1, t.row_of_ray, *t.brdf, *t.brdf_mask, d_brdf, g_mlp,
                                   below ? mlp_side_wgs : mlp_side_wgs_env, mlp_side, mlp_img());
            end_side();
            have_feat = true;
            keep_.push_back(d_brdf);
        }
        // ---- adjoint of the incoming radiance -> adjoint of the bounce rays [R,6]
        Tensor d_brays;
        if (!t.idx_re.has_value() && t.child) {
            d_brays = bwd(*t.child, d_inc, OT(), OT());
        } else if (!t.idx_re.has_value()) {
            d_brays = env_bwd(t.brays, t.mip, d_inc, main_stream);
        } else {
            d_brays = at::empty_like(t.brays);
            if (t.idx_re->size(0) > 0)
                d_brays.index_copy_(0, *t.idx_re, bwd(*t.child, at::index_select(d_inc, 0, *t.idx_re), OT(), OT()));
            if (t.idx_no->size(0) > 0)
                d_brays.index_copy_(0, *t.idx_no, env_bwd(*t.brays_no, *t.mip_no, at::index_select(d_inc, 0, *t.idx_no), main_stream));
        }
        if (lvl == 0 && last_chunk_ && used_env && d_bg_out.has_value()) {
            // every environment adjoint of the optimizer step has been queued: the two reverse prefix sums of the env-map table
            // run on a side stream from here (end_step picks the result up)
            const int64_t ss = fork(5);
            if (ss) {
                for (int64_t es : env_streams_)          // ... queued, not finished: the table adjoints still running on side streams
                    if (es != ss) side_waits_for(ss, es);
                for (int64_t ps : peer_streams)          // ... and the env adjoints of the chunks other contexts ran (joined into their mains)
                    if (ps != main_stream) side_waits_for(ss, ps);
                // (the table backward destroys the adjoint table it reads: a caller whose sum over chunks goes on -- the autograd
                //  node, which cannot know its last chunk -- has it run on a copy)
                Tensor ds = env_keep_sat ? d_sat.clone() : d_sat;
                sat_build_bwd_into(ds, env_bg, env_act, d_pole, 0.0, 1.0, env_sc, *d_bg_out, ss);
                if (env_keep_sat) keep_.push_back(ds);
                end_side();
                early_env_side_ = ss;
                early_env_done = true;
            }
        }
        if (mlp_side) join(mlp_side, {d_feat});
        if (!have_feat)
            d_feat = brdf_mlp_bwd(mlp_ws, t.hl, t.dl, t.feat, t.r1, t.row_of_ray, *t.brdf, *t.brdf_mask, d_brdf, g_mlp, 0, main_stream, mlp_img());
        Tensor dN, dr1, dV_ggx;
        if (view) {
            Tensor d_nrv = ggx_rays_bwd_view(t.V, t.N, t.r1, t.off, sobol, t.row_of_ray, t.j_of_ray, dL, d_brays, main_stream);
            Tensor rows7 = segment_sum_wide(d_nrv, 7, t.row_off, t.Mb, main_stream);
            dN = rows7.slice(1, 0, 3); dr1 = rows7.select(1, 3); dV_ggx = rows7.slice(1, 4, 7);
        } else {
            Tensor d_nr = ggx_rays_bwd(t.V, t.N, t.r1, t.off, sobol, t.row_of_ray, t.j_of_ray, dL, d_brays, main_stream);
            Tensor rows4 = segment_sum(d_nr, OT(), t.row_off, t.Mb, 8, main_stream);
            dN = rows4.slice(1, 0, 3); dr1 = rows4.select(1, 3);
        }
        Tensor d_normals, d_heads, d_app;
        if (t.sparse_n) {
            // the row preparation's adjoint inside the heads' backward: one launch per level instead of two on the main chain
            std::tie(d_normals, d_app) =
                bounce_prep_heads_bwd(t.bidx, *t.nr, t.heads, S.ray_id, S.rays, t.conv, min_rough, detach_n, dN, dr1, rows6.slice(1, 0, 3),
                                      rows6.slice(1, 3, 6), d_feat, t.app, head_W, head_b, head_p, g_hW, g_hb, main_stream);
        } else {
            std::tie(d_normals, d_heads, d_app) =
                bounce_prep_bwd(OT(t.inv), *t.nr, t.heads, S.ray_id, S.rays, t.conv, min_rough, detach_n, dN, dr1,
                                rows6.slice(1, 0, 3), rows6.slice(1, 3, 6), d_feat, t.bidx, 1, main_stream);
            d_app = heads_bwd(t.app, head_W, head_b, head_p, d_heads, g_hW, g_hb, OT(d_app), main_stream);
        }
        app_segs_.push_back(Seg(t.xyz_rows, OT(), OT(), OT(), OT(), OT(), d_app));
        OT d_normal;
        if (detach_n) d_normal = d_nrm;
        else if (d_nrm.has_value()) d_normal = d_normals.add_(*d_nrm);
        else d_normal = d_normals;
        if (t.sparse_n) {
            if (!early_walk) dens_segs_.push_back(Seg(S.xyzt, t.sf, OT(), d_sigma, OT(), OT(), OT()));
            if (d_normal.has_value())
                dens_segs_.push_back(Seg(t.xyz_rows, *t.sf_rows, *t.gr_rows, zero_like(*t.sf_rows), OT(), *d_normal, OT()));
        } else {
            dens_segs_.push_back(Seg(S.xyzt, t.sf, t.gr, d_sigma, OT(), d_normal, OT()));
        }
        if (env_side) join(env_side, {d_rays});
        if (view) {
            if (!d_rays.defined()) d_rays = at::zeros_like(S.rays);
            view_adjoint_to_rays(S.ray_id, t.bidx, dV_rows, dV_ggx, d_rays, main_stream);
        }
        return d_rays;
    }

    int64_t early_env_side_ = 0;
    // zeros that are only ever read (the sigma adjoint of a segment that carries none): one buffer instead of a fill per call
    Tensor zeros_, loss_ws_;
    Tensor zero_like(const Tensor& x) {
        const int64_t n = x.numel();
        if (!zeros_.defined() || zeros_.numel() < n || zeros_.device() != x.device())
            zeros_ = at::zeros({std::max<int64_t>(2 * n, 1 << 16)}, x.options().dtype(at::kFloat));
        return zeros_.narrow(0, 0, n).view(x.sizes());
    }

  public:
    // end_step: the main stream waits for the env-map table backward queued on the side stream
    void join_env_table_backward() {
        if (early_env_done && early_env_side_) join(early_env_side_);
        early_env_done = false;
        early_env_side_ = 0;
    }

  private:
    static std::vector<bool> seg_key(const Seg& s) {
        return {std::get<3>(s).has_value(), std::get<4>(s).has_value(), std::get<5>(s).has_value(), std::get<6>(s).has_value()};
    }
    void walk(std::vector<Seg>& all, const OT& gb, int64_t stream) {
        // one walk takes sample sets that carry the same adjoints
        std::vector<std::vector<bool>> keys;
        for (auto& s : all) {
            auto k = seg_key(s);
            if (std::find(keys.begin(), keys.end(), k) == keys.end()) keys.push_back(k);
        }
        for (auto& k : keys) {
            std::vector<Seg> segs;
            for (auto& s : all)
                if (seg_key(s) == k) segs.push_back(s);
            for (size_t i = 0; i < segs.size(); i += NMF_VM_MAX_SEGMENTS) {
                std::vector<Seg> part(segs.begin() + i, segs.begin() + std::min(segs.size(), i + (size_t)NMF_VM_MAX_SEGMENTS));
                walk_segments(part, gb, stream);
            }
        }
    }
    void flush_walks() {
        // (the appearance walk next to the density walk on a stream of its own: measured neutral twice, removed)
        walk(dens_segs_, OT(), main_stream);
        walk(app_segs_, g_basis, main_stream);
        for (int64_t s : walk_forks_) join(s);
        walk_forks_.clear();
        dens_segs_.clear();
        app_segs_.clear();
        keep_.clear();
    }
};
