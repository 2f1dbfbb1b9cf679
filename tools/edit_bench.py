"""Cost of the material edits: device time of one 800 x 800 frame of bench.py's S1 model (128^3) through render_images,
by HIP events, median (min / max) over N frames after three warm-up frames, and the two kernels stand-alone.
usage: python tools/edit_bench.py ROOT MODES [N]
  ROOT   the tree to import nmf_amd and bench from (this checkout: `.`; a built export of the parent commit for mode a)
  MODES  letters, in order: a = a tree without the edit API (the parent), b = no edits, c = one `all` edit (roughness * 0.4),
         d = 16 box edits, k = nmf_heads_edit on 2^20 rows and nmf_material_maps(_edit) on 16384 rays x ~20 samples
One JSON line per mode / kernel."""
import json
import os
import statistics
import sys

root = os.path.abspath(sys.argv[1])
modes = sys.argv[2]
N = int(sys.argv[3]) if len(sys.argv) > 3 else 24
sys.path.insert(0, root)
import torch  # noqa: E402

import bench  # noqa: E402
from nmf_amd import synthetic  # noqa: E402
from nmf_amd.noise import DeviceNoise  # noqa: E402
from nmf_amd.renderer import render_images  # noqa: E402

assert os.path.abspath(bench.__file__).startswith(root), bench.__file__
dev = torch.device("cuda", 0)
torch.manual_seed(3)
nerf, _ = bench.build(dev)
nerf.eval()
rays, focal = synthetic.camera_rays(0, all_pixels=True, wh=bench.FRAME)
rays = rays.to(dev)
chunk = nerf.eval_batch_size


def frames(label):
    noise = DeviceNoise(dev, seed=11)
    for _ in range(3):
        render_images(nerf, rays, focal, chunk, noise)
    torch.cuda.synchronize()
    ms = []
    for _ in range(N):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        render_images(nerf, rays, focal, chunk, noise)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    rec = dict(mode=label, root=os.path.relpath(root), frames=N, rays=int(rays.shape[0]), chunk=int(chunk),
               median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))
    print(json.dumps(rec), flush=True)


def timed(fn, n=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


for m in modes:
    if m in "ab":
        frames(m)
    elif m in "cd":
        from nmf_amd import edit as E
        if m == "c":
            edits = [E.MaterialEdit.scale("roughness", 0.4)]
        else:
            edits = [E.MaterialEdit.set(E.TARGETS[i % 3], 0.2 + 0.04 * i, E.Region.box((0.1 * (i % 5) - 0.2, 0.05 * i - 0.4, 0.0), (0.3, 0.25, 0.5)),
                                        falloff=0.05 * (i % 2)) for i in range(16)]
        nerf.set_material_edits(edits)
        frames(m)
        nerf.set_material_edits(None)
    elif m == "k":
        from nmf_amd import edit as E
        from nmf_amd import hip
        n = 1 << 20
        heads = torch.rand(n, 11, device=dev) * 0.9 + 0.05
        xyzt = torch.rand(n, 4, device=dev) * 3 - 1.5
        one = E.pack([E.MaterialEdit.scale("roughness", 0.4)])
        boxes = E.pack([E.MaterialEdit.set(E.TARGETS[i % 3], 0.2 + 0.04 * i, E.Region.box((0.1 * (i % 5) - 0.2, 0.05 * i - 0.4, 0.0), (0.3, 0.25, 0.5)),
                                           falloff=0.05 * (i % 2)) for i in range(16)])
        for label, tab in (("heads_edit K=1", one), ("heads_edit K=16", boxes)):
            med, lo, hi = timed(lambda: hip.heads_edit(heads, xyzt, tab))
            byts = n * (2 * 44 + 16)
            print(json.dumps(dict(kernel=label, rows=n, median_us=round(med * 1e3, 2), min_us=round(lo * 1e3, 2), max_us=round(hi * 1e3, 2),
                                  bytes=byts, GBps=round(byts / (med * 1e-3) / 1e9, 1))), flush=True)
        B = 16384
        g = torch.Generator().manual_seed(1)
        u = lambda *sh: torch.rand(*sh, generator=g)                                     # noqa: E731
        cnt = torch.randint(10, 32, (B,), generator=g)
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)])
        M = int(offsets[-1])
        has = torch.zeros(M, dtype=torch.bool)
        has[::3] = True
        Mb = int(has.sum())
        inv = torch.full((M,), -1, dtype=torch.int32)
        inv[has] = torch.arange(Mb, dtype=torch.int32)
        rc = torch.randint(0, 4, (Mb,), generator=g)
        row_off = torch.cat([torch.zeros(1, dtype=torch.int64), rc.cumsum(0)])
        R = int(row_off[-1])
        w = u(M) / 20
        c = dict(app=u(M, 24) * 2 - 1, normals=torch.nn.functional.normalize(u(M, 3) * 2 - 1, dim=-1), weight=w, offsets=offsets,
                 rays=torch.cat([u(B, 3), torch.nn.functional.normalize(u(B, 3) * 2 - 1, dim=-1)], -1), head_W=u(11, 24) - 0.5,
                 head_b=u(11) - 0.5, conv=u(9, 3), acc=torch.zeros(B).index_add_(0, torch.repeat_interleave(torch.arange(B), cnt), w),
                 bg=torch.ones(3), inv=inv, row_off=row_off, cnt=rc.int(), incoming=u(R, 3), brdf_weight=u(R, 3),
                 xyzt=torch.cat([u(M, 3) * 3 - 1.5, u(M, 1)], -1))
        c = {k: v.to(dev).contiguous() for k, v in c.items()}
        hp = (1.3, -0.2, 0.1, -0.4, 0.3)

        def _maps(c, hp, **kw):
            return hip.material_maps(c["app"], c["normals"], c["weight"], c["offsets"], c["rays"], c["head_W"], c["head_b"], hp, c["conv"],
                                     c["acc"], c["bg"], c["inv"], c["row_off"], c["cnt"], c["incoming"], c["brdf_weight"], **kw)
        byts = M * (96 + 12 + 4 + 4 + 16) + B * (24 + 8 + 4 + 60) + int(c["incoming"].shape[0]) * 24
        for label, kw in (("material_maps", {}), ("material_maps_edit K=0", dict(xyz=c["xyzt"], edits=None)),
                          ("material_maps_edit K=1", dict(xyz=c["xyzt"], edits=one)), ("material_maps_edit K=16", dict(xyz=c["xyzt"], edits=boxes))):
            med, lo, hi = timed(lambda: _maps(c, hp, **kw))
            print(json.dumps(dict(kernel=label, rays=B, samples=M, median_us=round(med * 1e3, 2), min_us=round(lo * 1e3, 2),
                                  max_us=round(hi * 1e3, 2), bytes=byts, GBps=round(byts / (med * 1e-3) / 1e9, 1))), flush=True)
