"""Mesh export entry point -- counterpart of the reference's scripts/export_mesh.py for checkpoints written by TensorNeRF.save:

    python -m nmf_amd.export_mesh --ckpt log/lego.th [--resolution 512] [--level 0.005] [--no-attributes] [--reference-spacing]
                                  [--output lego.ply]

Marching cubes of the alpha lattice on the GPU (nmf_amd/mesh.py); every vertex carries the field's normal, the albedo as sRGB colour,
roughness and f0 unless --no-attributes.  The default output is the checkpoint path with .th replaced by .ply, as the reference
names it.  --reference-spacing places the vertices as the reference does (shrunk by (G - 1) / G, see nmf_amd/mesh.py).
Prints one JSON line: V, F and the seconds per stage (density sweep, triangulation, attributes, PLY write).
"""
import argparse
import json
import os
import time

import torch


def default_output(ckpt):
    return ckpt[:-3] + ".ply" if ckpt.endswith(".th") else ckpt + ".ply"


def export(nerf, path, resolution=None, level=0.005, attributes=True, reference_spacing=False):
    """extract_mesh + write_ply -> the record the command line prints"""
    from .mesh import extract_mesh, write_ply
    mesh = extract_mesh(nerf, resolution=resolution, level=level, attributes=attributes, reference_spacing=reference_spacing)
    t0 = time.perf_counter()
    write_ply(path, mesh)
    sec = dict(mesh.seconds, write=time.perf_counter() - t0)
    return dict(output=path, V=int(mesh.verts.shape[0]), F=int(mesh.faces.shape[0]), attributes=bool(attributes),
                seconds={k: round(v, 4) for k, v in sec.items()})


def main(argv=None):
    ap = argparse.ArgumentParser(description="Export the alpha iso-surface of a checkpoint as a PLY mesh (GPU marching cubes).")
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--resolution", type=int, nargs="+", default=None,
                    help="lattice points per axis, one value or three (default: the field's grid size)")
    ap.add_argument("--level", type=float, default=0.005, help="alpha iso-level (the reference's 0.005)")
    ap.add_argument("--no-attributes", action="store_true", help="positions and faces only, the reference's file layout")
    ap.add_argument("--reference-spacing", action="store_true",
                    help="place the vertices as the reference does: aabb[0] + idx * size / G instead of size / (G - 1)")
    ap.add_argument("--output", default=None, help="default: the checkpoint path with .th replaced by .ply")
    from . import edit
    edit.add_arguments(ap)
    args = ap.parse_args(argv)
    if args.resolution is not None and len(args.resolution) not in (1, 3):
        ap.error("--resolution takes one value or three")
    try:
        material_edits = edit.from_args(args)
    except (edit.EditError, OSError) as e:
        ap.error(str(e))
    from .modules.tensor_nerf import TensorNeRF
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    nerf = TensorNeRF.load(args.ckpt, device=dev)
    nerf.eval()
    nerf.set_material_edits(material_edits)          # the vertex attributes carry the edited materials
    res = None if args.resolution is None else (args.resolution[0] if len(args.resolution) == 1 else args.resolution)
    rec = export(nerf, args.output or default_output(args.ckpt), res, args.level, not args.no_attributes, args.reference_spacing)
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    main()
