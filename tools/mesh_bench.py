"""Stage times of the mesh export on bench.py's S1 model at lattice resolutions 128, 300 and 512: density sweep
(AlphaGridSampler.getDenseAlpha), count pass, scan (two int64 totals, two in-place cumsums, the read-back), emit pass, vertex
attributes -- HIP events around each stage -- and the PLY write (wall clock).  One warm-up export per resolution, then `reps` timed
ones; prints per stage the median, min and max ms and its share of the whole export, and for the count pass the bytes it must
read (4 Gx Gy Gz) over its median time as a fraction of the 6.29 TB/s copy rate of DESIGN.md.  --texture-size W adds the texture bake
of the same mesh (mesh.bake_textures: texel placement, field queries, store -- HIP events summed over the chunks -- and its wall time) and
the OBJ + MTL + PNG write (wall clock), and for the two atlas kernels the bytes they move over their time against the same copy rate.
    python tools/mesh_bench.py [--texture-size W] [reps] [resolution ...]      (default 5 reps; 128 300 512)"""
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402
from nmf_amd import hip  # noqa: E402
from nmf_amd.mesh import Mesh, bake_textures, vertex_attributes, write_obj, write_ply  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s, DESIGN.md section 6
LEVEL = 0.005
STAGES = ("density", "count", "scan", "emit", "attributes")

args = sys.argv[1:]
texture_size = None
if "--texture-size" in args:
    k = args.index("--texture-size")
    texture_size = int(args[k + 1])
    del args[k:k + 2]
BAKE_STAGES = ("texels", "queries", "store")
reps = int(args.pop(0)) if args else 5
resolutions = [int(a) for a in args] or [128, 300, 512]
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
nerf, _ = bench.build(dev)
nerf.eval()


def export(G, path):
    """one export with an event between the stages -> ({stage: ms}, V, F)"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
    with torch.no_grad():
        ev[0].record()
        alpha = nerf.sampler.getDenseAlpha(nerf.rf, [G] * 3)
        ev[1].record()
        cases, vcount, tcount = hip.mc_count(alpha, LEVEL)
        ev[2].record()
        rb = hip.Readback.of(dev).start(torch.stack([vcount.sum(), tcount.sum()]))
        torch.cumsum(vcount, 0, dtype=torch.int32, out=vcount)
        torch.cumsum(tcount, 0, dtype=torch.int32, out=tcount)
        V, F = rb.get()
        ev[3].record()
        idx, faces = hip.mc_emit(alpha, LEVEL, cases, vcount, tcount, V, F)
        ev[4].record()
        aabb = nerf.sampler.aabb.to(dev).float()
        verts = aabb[0] + idx * ((aabb[1] - aabb[0]) / (G - 1))
        mesh = Mesh(verts, faces, *vertex_attributes(nerf, verts))
        ev[5].record()
    torch.cuda.synchronize()
    ms = {s: ev[i].elapsed_time(ev[i + 1]) for i, s in enumerate(STAGES)}
    t0 = time.perf_counter()
    write_ply(path, mesh)
    ms["write"] = (time.perf_counter() - t0) * 1e3
    if texture_size is not None:
        tex = bake_textures(nerf, mesh, size=texture_size)
        for k in BAKE_STAGES:
            ms["bake_" + k] = tex.seconds[k] * 1e3
        ms["bake_wall"] = tex.seconds["bake"] * 1e3
        t0 = time.perf_counter()
        write_obj(path[:-4] + ".obj", mesh, tex)
        ms["write_obj"] = (time.perf_counter() - t0) * 1e3
        print(f"# {G}^3 with a {texture_size}^2 atlas: one export done", file=sys.stderr, flush=True)      # (a 512^3 / 8192^2 one takes a while)
        ms["_layout"], ms["_owned"] =tex.layout, int((tex.normal.view(-1, 3) != 128).any(dim=1).sum())
    return ms, V, F


with tempfile.TemporaryDirectory() as tmp:
    for G in resolutions:
        path = os.path.join(tmp, f"g{G}.ply")
        export(G, path)                                                           # warm-up: code objects, allocator, tables
        runs = [export(G, path) for _ in range(reps)]
        V, F = runs[0][1], runs[0][2]
        med = {s: statistics.median(r[0][s] for r in runs) for s in STAGES + ("write",)}
        total = sum(med.values())
        rec = dict(resolution=G, V=V, F=F, reps=reps, ply_bytes=os.path.getsize(path), total_ms=round(total, 3), stages={})
        for s in STAGES + ("write",):
            t = [r[0][s] for r in runs]
            rec["stages"][s] = dict(median_ms=round(med[s], 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                                    share=round(med[s] / total, 4))
        rate = 4.0 * G ** 3 / (med["count"] * 1e-3)
        rec["count_read_bytes"] = 4 * G ** 3
        rec["count_read_rate_TBps"] = round(rate / 1e12, 4)
        rec["count_fraction_of_copy_rate"] = round(rate / COPY_RATE, 4)
        if texture_size is not None:
            W, T = runs[0][0]["_layout"][:2]
            owned = runs[0][0]["_owned"]          # (texels whose normal byte triple is not the fill: every owned one but an exact zero normal)
            rec.update(texture_size=W, texels_per_square=T, owned_texels=owned, bake={})
            for s in tuple("bake_" + k for k in BAKE_STAGES) + ("bake_wall", "write_obj"):
                t = [r[0][s] for r in runs]
                rec["bake"][s] = dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))
            # texel placement writes 16 B per texel (position + owner); the store reads the owner of every texel and 40 B of attributes
            # per owned one and writes 10 B per texel
            moved = dict(bake_texels=16 * W * W, bake_store=(4 + 10) * W * W + 40 * owned)
            for s, b in moved.items():
                rate = b / (rec["bake"][s]["median_ms"] * 1e-3)
                rec["bake"][s].update(bytes=b, rate_TBps=round(rate / 1e12, 4), fraction_of_copy_rate=round(rate / COPY_RATE, 4))
        print(json.dumps(rec), flush=True)
