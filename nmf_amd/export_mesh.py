"""Mesh export entry point -- counterpart of the reference's scripts/export_mesh.py for checkpoints written by TensorNeRF.save:

    python -m nmf_amd.export_mesh --ckpt log/lego.th [--resolution 512] [--level 0.005] [--no-attributes] [--reference-spacing]
                                  [--texture-size 4096] [--output lego.ply]

Marching cubes of the alpha lattice on the GPU (nmf_amd/mesh.py); every vertex carries the field's normal, the albedo as sRGB colour,
roughness and f0 unless --no-attributes.  The default output is the checkpoint path with .th replaced by .ply, as the reference
names it.  --reference-spacing places the vertices as the reference does (shrunk by (G - 1) / G, see nmf_amd/mesh.py).
--texture-size W bakes albedo, f0, roughness and world-space normals into a W x W per-triangle texture atlas instead
(mesh.bake_textures) and writes <name>.obj, <name>.mtl and four PNGs (default name: the checkpoint path without .th): --resolution
picks the triangle count, --texture-size the material detail.
Prints one JSON line: V, F and the seconds per stage (density sweep, triangulation, attributes, [bake,] file write).
"""
import argparse
import json
import os
import time

import torch


def default_output(ckpt, ext=".ply"):
    return ckpt[:-3] + ext if ckpt.endswith(".th") else ckpt + ext


def export(nerf, path, resolution=None, level=0.005, attributes=True, reference_spacing=False, texture_size=None):
    """extract_mesh + write_ply (texture_size: + bake_textures, and write_obj in place of write_ply) -> the record the command line
    prints"""
    from .mesh import bake_textures, extract_mesh, write_obj, write_ply
    if texture_size is not None and not attributes:
        raise ValueError("export: a texture atlas holds the attributes, texture_size and attributes=False exclude each other")
    mesh = extract_mesh(nerf, resolution=resolution, level=level, attributes=attributes, reference_spacing=reference_spacing)
    sec, extra = dict(mesh.seconds), {}
    if texture_size is not None:
        tex = bake_textures(nerf, mesh, size=texture_size)
        sec["bake"] = tex.seconds["bake"]
        extra = dict(texture_size=tex.layout[0], texels_per_square=tex.layout[1])
    t0 = time.perf_counter()
    if texture_size is not None:
        path = write_obj(path, mesh, tex)["obj"]
    else:
        write_ply(path, mesh)
    sec["write"] = time.perf_counter() - t0
    return dict(output=path, V=int(mesh.verts.shape[0]), F=int(mesh.faces.shape[0]), attributes=bool(attributes), **extra,
                seconds={k: round(v, 4) for k, v in sec.items()})


def main(argv=None):
    ap = argparse.ArgumentParser(description="Export the alpha iso-surface of a checkpoint as a PLY mesh (GPU marching cubes), or "
                                             "as an OBJ with baked material textures (--texture-size).")
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--resolution", type=int, nargs="+", default=None,
                    help="lattice points per axis, one value or three (default: the field's grid size)")
    ap.add_argument("--level", type=float, default=0.005, help="alpha iso-level (the reference's 0.005)")
    ap.add_argument("--no-attributes", action="store_true", help="positions and faces only, the reference's file layout")
    ap.add_argument("--reference-spacing", action="store_true",
                    help="place the vertices as the reference does: aabb[0] + idx * size / G instead of size / (G - 1)")
    ap.add_argument("--texture-size", type=int, default=None, metavar="W",
                    help="bake albedo, f0, roughness and world-space normals into a W x W per-triangle atlas (4..16384) and write "
                         "OBJ + MTL + PNGs instead of a PLY")
    ap.add_argument("--output", default=None, help="default: the checkpoint path with .th replaced by .ply (.obj with --texture-size)")
    from . import edit
    edit.add_arguments(ap)
    args = ap.parse_args(argv)
    if args.resolution is not None and len(args.resolution) not in (1, 3):
        ap.error("--resolution takes one value or three")
    if args.texture_size is not None:
        from .mesh import ATLAS_MAX, ATLAS_MIN
        if args.no_attributes:
            ap.error("--no-attributes and --texture-size exclude each other (the textures hold the attributes)")
        if not ATLAS_MIN <= args.texture_size <= ATLAS_MAX:
            ap.error(f"--texture-size is {ATLAS_MIN}..{ATLAS_MAX}, got {args.texture_size}")
    try:
        material_edits = edit.from_args(args)
    except (edit.EditError, OSError) as e:
        ap.error(str(e))
    from .modules.tensor_nerf import TensorNeRF
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    nerf = TensorNeRF.load(args.ckpt, device=dev)
    nerf.eval()
    nerf.set_material_edits(material_edits)          # the vertex attributes and the baked textures carry the edited materials
    res = None if args.resolution is None else (args.resolution[0] if len(args.resolution) == 1 else args.resolution)
    out = args.output or default_output(args.ckpt, ".ply" if args.texture_size is None else ".obj")
    rec = export(nerf, out, res, args.level, not args.no_attributes, args.reference_spacing, args.texture_size)
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    main()
