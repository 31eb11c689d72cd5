"""Mesh export of a trained field: scripts/export_mesh.py:15-24 -> utils.py:164-226 (convert_sdf_samples_to_ply), on the device.

    verts, faces, normals = extract_mesh(model)          # dense alpha lattice -> marching cubes (tir_dense_alpha, tir_mc_*)
    export_mesh(model, "scene.ply")                      # + binary PLY, laid out as plyfile writes the reference's mesh

Coordinates follow the reference, quirk included (Appendix B policy: parity first): convert_sdf_samples_to_ply takes the voxel
size as (aabb[1] - aabb[0]) / shape -- `shape`, not `shape - 1` (utils.py:186) -- although getDenseAlpha's lattice spans the
aabb with linspace(0, 1, g).  Its mesh is therefore the true surface scaled by (g - 1) / g toward aabb[0].  extract_mesh keeps
that scale and has no option for it; a caller who wants lattice-exact positions calls ops.marching_cubes with
spacing (aabb[1] - aabb[0]) / (g - 1) directly.  Faces are written in the reference's final orientation: outward (from high
alpha to low), which is the kernel's own winding (the reference reverses scikit-image's, utils.py:191).
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

# numpy dtype -> PLY scalar type names, as plyfile spells them
_PLY_TYPES = {"f4": "float", "f8": "double", "i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int",
              "u4": "uint"}


def _ply_type(dt):
    key = dt.base.kind + str(dt.base.itemsize)
    if key not in _PLY_TYPES:
        raise ValueError(f"no PLY type for {dt}")
    return _PLY_TYPES[key]


def write_elements(path, elements):
    """Binary little-endian PLY of named structured arrays [(name, array), ...].  A scalar field is a `property <type> name`, a
    fixed-size subarray field a `property list uchar <type> name` (the count byte is written before every row), which is how
    plyfile describes the reference's arrays.  One header, one pass over the data; no per-row Python loop."""
    header = ["ply", "format binary_little_endian 1.0"]
    bodies = []
    for name, arr in elements:
        arr = np.asarray(arr)
        header.append(f"element {name} {len(arr)}")
        fields = []
        for fname in arr.dtype.names:
            dt = arr.dtype.fields[fname][0]
            le = dt.base.newbyteorder("<")
            if dt.shape:
                if len(dt.shape) != 1 or dt.shape[0] > 255:
                    raise ValueError(f"{name}.{fname}: list properties take one axis of at most 255 entries")
                header.append(f"property list uchar {_ply_type(dt)} {fname}")
                fields += [(fname + "__count", "u1"), (fname, le, dt.shape)]
            else:
                header.append(f"property {_ply_type(dt)} {fname}")
                fields.append((fname, le))
        rec = np.empty(len(arr), dtype=np.dtype(fields))      # packed (no alignment padding), little-endian
        for fname in arr.dtype.names:
            dt = arr.dtype.fields[fname][0]
            if dt.shape:
                rec[fname + "__count"] = dt.shape[0]
            rec[fname] = arr[fname]
        bodies.append(rec.tobytes())
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        for b in bodies:
            f.write(b)


def write_ply(path, verts, faces):
    """verts [V, 3] float32 positions, faces [F, 3] int32 vertex indices -> binary little-endian PLY with
    `element vertex V` / `property float x|y|z` / `element face F` / `property list uchar int vertex_indices`."""
    verts = np.asarray(verts.cpu() if torch.is_tensor(verts) else verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces.cpu() if torch.is_tensor(faces) else faces, np.int32).reshape(-1, 3)
    v = np.empty(len(verts), dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])
    v["x"], v["y"], v["z"] = verts[:, 0], verts[:, 1], verts[:, 2]
    f = np.empty(len(faces), dtype=[("vertex_indices", "i4", (3,))])
    f["vertex_indices"] = faces
    write_elements(path, [("vertex", v), ("face", f)])


def read_ply(path):
    """The inverse of write_ply (for files laid out exactly as it writes them) -> (verts [V, 3] f32, faces [F, 3] i32)."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    nv = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[2])
    nf = int(next(ln for ln in lines if ln.startswith("element face")).split()[2])
    v = np.frombuffer(data, dtype="<f4", count=3 * nv, offset=end).reshape(nv, 3)
    f = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=nf, offset=end + 12 * nv)
    if nf and not (f["n"] == 3).all():
        raise ValueError("read_ply: only triangle faces are supported")
    return v.astype(np.float32), f["i"].astype(np.int32)


def reference_spacing(aabb, grid):
    """utils.py:186: (aabb[1] - aabb[0]) / shape in fp32 (the reference divides a float32 tensor by the integer shape)."""
    aabb = torch.as_tensor(aabb).detach().to("cpu", torch.float32)
    return ((aabb[1] - aabb[0]) / torch.tensor([float(g) for g in grid], dtype=torch.float32)).tolist()


@torch.no_grad()
def extract_mesh(model, level=0.005, gridSize=None):
    """getDenseAlpha(gridSize) (default: the model's gridSize) -> marching cubes at `level` in the reference's coordinates
    (module docstring).  -> (verts [V, 3] f32, faces [F, 3] i32 outward, normals [V, 3] f32), on the model's device."""
    grid = [int(g) for g in (model.gridSize if gridSize is None else gridSize)]
    alpha, _ = ops.dense_alpha(model.packed_field(), grid, float(model.stepSize))   # getDenseAlpha's alpha, no xyz lattice
    aabb = model.aabb.detach().to("cpu", torch.float32)
    return ops.marching_cubes(alpha, level, reference_spacing(aabb, grid), aabb[0].tolist())


@torch.no_grad()
def export_mesh(model, path, level=0.005, gridSize=None):
    """extract_mesh + write_ply -> (number of vertices, number of faces)."""
    verts, faces, _ = extract_mesh(model, level, gridSize)
    write_ply(path, verts, faces)
    return verts.shape[0], faces.shape[0]
