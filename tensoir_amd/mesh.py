"""Mesh export of a trained field: scripts/export_mesh.py:15-24 -> utils.py:164-226 (convert_sdf_samples_to_ply), on the device.

    verts, faces, normals = extract_mesh(model)          # dense alpha lattice -> marching cubes (tir_dense_alpha, tir_mc_*)
    extract_mesh(model, keep_largest=1)                  # ... without the detached blobs ("floaters"): tir_ccl_* on the lattice
    export_mesh(model, "scene.ply")                      # + binary PLY, laid out as plyfile writes the reference's mesh
    export_mesh(model, "scene.ply", attributes=True)     # + per-vertex materials and direct lighting (tensoir_amd/bake.py)
    export_mesh(model, "scene.ply", simplify=3)          # a face budget: one vertex per 3 x 3 x 3 block of cells (tir_simplify_*)

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


_PLY_DTYPES = {v: k for k, v in _PLY_TYPES.items()}
_PLY_DTYPES.update({"float32": "f4", "float64": "f8", "int8": "i1", "uint8": "u1", "int16": "i2", "uint16": "u2", "int32": "i4",
                    "uint32": "u4"})


def read_ply_attributes(path):
    """A binary little-endian PLY with a `vertex` element of scalar properties (x y z first) followed by a `face` element of one
    triangle list property, as write_elements lays them out -> (verts [V, 3] f32, faces [F, 3] i32, {property: [V] array} of the
    vertex properties other than x y z, in their file types; empty for a plain file)."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("read_ply_attributes: only binary little-endian PLY files are supported")
    elements = []                                             # [name, count, [(property, dtype) or (property, count type, dtype)]]
    for ln in lines[2:]:
        t = ln.split()
        if not t or t[0] in ("comment", "obj_info", "end_header"):
            continue
        if t[0] == "element":
            elements.append([t[1], int(t[2]), []])
        elif t[0] == "property" and elements:
            if t[1] == "list":
                elements[-1][2].append((t[4], "<" + _PLY_DTYPES[t[2]], "<" + _PLY_DTYPES[t[3]]))
            else:
                elements[-1][2].append((t[2], "<" + _PLY_DTYPES[t[1]]))
        else:
            raise ValueError(f"read_ply_attributes: unexpected header line {ln!r}")
    if [e[0] for e in elements] != ["vertex", "face"]:
        raise ValueError("read_ply_attributes: expected a vertex element followed by a face element")
    (_, nv, vprops), (_, nf, fprops) = elements
    if any(len(p) != 2 for p in vprops) or [p[0] for p in vprops[:3]] != ["x", "y", "z"]:
        raise ValueError("read_ply_attributes: vertex properties must be scalars starting with x y z")
    if len(fprops) != 1 or len(fprops[0]) != 3:
        raise ValueError("read_ply_attributes: the face element takes one list property")
    vdt = np.dtype([(n, t) for n, t in vprops])
    v = np.frombuffer(data, dtype=vdt, count=nv, offset=end)
    fdt = np.dtype([("n", fprops[0][1]), ("i", fprops[0][2], (3,))])
    f = np.frombuffer(data, dtype=fdt, count=nf, offset=end + vdt.itemsize * nv)
    if nf and not (f["n"] == 3).all():
        raise ValueError("read_ply_attributes: only triangle faces are supported")
    verts = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float32) if nv else np.zeros((0, 3), np.float32)
    attrs = {n: np.ascontiguousarray(v[n]).astype(np.dtype(t).newbyteorder("=")) for n, t in vprops[3:]}
    return verts, f["i"].astype(np.int32).reshape(-1, 3), attrs


# the vertex element of export_mesh(..., attributes=True): property -> numpy type, in file order
ATTRIBUTE_LAYOUT = ([(n, "f4") for n in ("x", "y", "z", "nx", "ny", "nz")] + [(n, "u1") for n in ("red", "green", "blue")] +
                    [(n, "f4") for n in ("roughness", "ao", "coverage", "albedo_r", "albedo_g", "albedo_b", "irradiance_r",
                                         "irradiance_g", "irradiance_b")])


def field_positions(aabb, grid, verts, normals=None):
    """Where the field must be queried for the vertices of extract_mesh / export_mesh.  The file keeps the reference's voxel-size
    quirk (module docstring): lattice point idx is written at aabb0 + idx * (aabb1 - aabb0) / g, while the lattice the alpha
    values were sampled on places it at aabb0 + idx * (aabb1 - aabb0) / (g - 1).  -> aabb0 + (v - aabb0) * g / (g - 1) per axis.
    normals (marching cubes': unit, in INDEX space) -> additionally the world directions normalize(n_idx / spacing) with the true
    lattice spacing (aabb1 - aabb0) / (g - 1): a gradient per index step is a gradient per `spacing` of world length."""
    verts = torch.as_tensor(verts)
    dev = verts.device
    box = torch.as_tensor(aabb).detach().to(dev, torch.float32).reshape(2, 3)
    g = torch.tensor([float(x) for x in grid], dtype=torch.float32, device=dev)
    pos = box[0] + (verts.to(torch.float32) - box[0]) * (g / (g - 1))
    if normals is None:
        return pos
    n = torch.as_tensor(normals).to(dev, torch.float32) / ((box[1] - box[0]) / (g - 1))
    return pos, n / torch.linalg.norm(n, dim=-1, keepdim=True).clamp(min=1e-20)


def vertex_colors(albedo, irradiance=None, color="albedo"):
    """[V, 3] uint8 display colours of baked vertices: round(255 * linear2srgb(c)) with c = albedo, or the Lambertian radiance
    clamp(albedo / pi * irradiance, 0, 1) under the baked light (color="diffuse")."""
    from .relight import linear2srgb_torch
    if color == "albedo":
        c = albedo
    elif color == "diffuse":
        if irradiance is None:
            raise ValueError('color="diffuse" needs the baked irradiance (lighting=True)')
        c = (albedo / np.pi * irradiance).clamp(0, 1)
    else:
        raise ValueError(f"color: 'albedo' or 'diffuse', not {color!r}")
    return torch.round(255.0 * linear2srgb_torch(c)).clamp(0, 255).to(torch.uint8)


def reference_spacing(aabb, grid):
    """utils.py:186: (aabb[1] - aabb[0]) / shape in fp32 (the reference divides a float32 tensor by the integer shape)."""
    aabb = torch.as_tensor(aabb).detach().to("cpu", torch.float32)
    return ((aabb[1] - aabb[0]) / torch.tensor([float(g) for g in grid], dtype=torch.float32)).tolist()


def select_components(table, keep_largest=None, min_voxels=None):
    """Which components of ops.label_components' table to keep -> [K] bool on the table's device.  A host policy on the small
    table: keep_largest=n keeps the n largest (ties go to the smaller root, i.e. the earlier row), min_voxels=m those with at
    least m voxels; with both, a component must pass both; with neither, all are kept."""
    for name, v, lo in (("keep_largest", keep_largest, 0), ("min_voxels", min_voxels, 0)):
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name}: expected an integer or None, not {v!r}")
        if v < lo:
            raise ValueError(f"{name}: must be >= {lo}, not {v}")
    sizes = torch.as_tensor(table["sizes"])
    if sizes.dim() != 1:
        raise ValueError(f"table['sizes']: expected [K], got {tuple(sizes.shape)}")
    host = sizes.detach().cpu().numpy().astype(np.int64)
    keep = np.ones(host.shape[0], dtype=bool)
    if min_voxels is not None:
        keep &= host >= int(min_voxels)
    if keep_largest is not None:
        order = np.argsort(-host, kind="stable")              # stable: equal sizes stay in root order
        top = np.zeros_like(keep)
        top[order[:int(keep_largest)]] = True
        keep &= top
    return torch.from_numpy(keep).to(sizes.device)


def _check_component_options(keep_largest, min_component_voxels, connectivity):
    """-> True when a component filter was asked for.  Raises before anything touches the device."""
    if connectivity not in (6, 26):
        raise ValueError(f"connectivity: 6 or 26, not {connectivity!r}")
    select_components({"sizes": torch.zeros(0, dtype=torch.int32)}, keep_largest, min_component_voxels)
    return keep_largest is not None or min_component_voxels is not None


def _check_simplify(simplify):
    """-> the cluster size k, or None.  Raises before anything touches the device."""
    if simplify is None:
        return None
    if isinstance(simplify, bool) or not isinstance(simplify, (int, np.integer)):
        raise ValueError(f"simplify: expected an integer >= 2 or None, not {simplify!r}")
    if simplify < 2:
        raise ValueError(f"simplify: must be >= 2, not {simplify}")
    return int(simplify)


def simplify_extracted(verts, faces, aabb, grid, k, reg=1e-2):
    """ops.simplify_mesh on a mesh of extract_mesh with clusters of k x k x k marching-cubes cells: cell = k *
    reference_spacing, origin = aabb[0], dims = (g - 1) // k + 1.  -> (verts', faces', INDEX-space unit normals, cell_of_vertex);
    the normals are normalize(n' * reference_spacing), what field_positions expects of marching cubes' own."""
    aabb = torch.as_tensor(aabb).detach().to("cpu", torch.float32).reshape(2, 3)
    sp = torch.tensor(reference_spacing(aabb, grid), dtype=torch.float32)
    cell = (sp * float(k)).tolist()
    v, f, n, cov = ops.simplify_mesh(verts, faces, cell, aabb[0].tolist(), [(int(g) - 1) // k + 1 for g in grid], reg)
    n = n * sp.to(n.device)
    return v, f, n / torch.linalg.norm(n, dim=-1, keepdim=True).clamp(min=1e-20), cov


def _model_grid(model, gridSize):
    return [int(g) for g in (model.gridSize if gridSize is None else gridSize)]


@torch.no_grad()
def components(model, level=0.005, gridSize=None, connectivity=6):
    """The component table of the model's alpha lattice (getDenseAlpha at gridSize, default the model's) at `level`, for
    inspection before choosing keep_largest / min_component_voxels: ops.label_components' table plus "boxes_world" [K, 2, 3]
    f32, the boxes in world coordinates of the TRUE lattice (spacing (aabb1 - aabb0) / (g - 1); a one-point axis sits at
    aabb0) -- not the reference's scaled mesh coordinates (module docstring)."""
    _check_component_options(None, None, connectivity)
    grid = _model_grid(model, gridSize)
    alpha, _ = ops.dense_alpha(model.packed_field(), grid, float(model.stepSize))
    _, table = ops.label_components(alpha, level, connectivity)
    box = model.aabb.detach().to(alpha.device, torch.float32).reshape(2, 3)
    g = torch.tensor([float(x) for x in grid], dtype=torch.float32, device=alpha.device)
    spacing = (box[1] - box[0]) / (g - 1).clamp(min=1.0)
    table["boxes_world"] = box[0] + table["boxes"].to(torch.float32).view(-1, 2, 3) * spacing
    return table


def _filtered_alpha(alpha, level, keep_largest, min_component_voxels, connectivity):
    """dense alpha -> (alpha without the components the selection drops, table, kept flags)."""
    labels, table = ops.label_components(alpha, level, connectivity)
    kept = select_components(table, keep_largest, min_component_voxels)
    return ops.keep_components(alpha, labels, table, kept, fill=0.0, level=level), table, kept


@torch.no_grad()
def extract_mesh(model, level=0.005, gridSize=None, *, keep_largest=None, min_component_voxels=None, connectivity=6,
                 report=None, simplify=None):
    """getDenseAlpha(gridSize) (default: the model's gridSize) -> marching cubes at `level` in the reference's coordinates
    (module docstring).  -> (verts [V, 3] f32, faces [F, 3] i32 outward, normals [V, 3] f32), on the model's device.
    keep_largest / min_component_voxels (select_components): the lattice's components under `connectivity` that fail the
    selection are set to 0 before marching cubes.  With connectivity 6 that removes whole closed surfaces and leaves every kept
    vertex bit-identical.  Needs level >= 0.  With both None no labelling kernel runs.
    simplify=k (an integer >= 2): the mesh is then reduced by quadric vertex clustering over blocks of k x k x k marching-cubes
    cells (simplify_extracted; the component filter runs first, on the lattice); the normals are the clusters' summed face
    normals in index space.  report (a dict) receives "full" = (vertices, faces) before the reduction.  With None no
    simplification kernel runs."""
    filtering = _check_component_options(keep_largest, min_component_voxels, connectivity)
    k = _check_simplify(simplify)
    grid = _model_grid(model, gridSize)
    alpha, _ = ops.dense_alpha(model.packed_field(), grid, float(model.stepSize))   # getDenseAlpha's alpha, no xyz lattice
    if filtering:
        alpha, table, kept = _filtered_alpha(alpha, level, keep_largest, min_component_voxels, connectivity)
        if report is not None:
            report.update(table=table, kept=kept)
    aabb = model.aabb.detach().to("cpu", torch.float32)
    verts, faces, normals = ops.marching_cubes(alpha, level, reference_spacing(aabb, grid), aabb[0].tolist())
    if k is None:
        return verts, faces, normals
    if report is not None:
        report["full"] = (verts.shape[0], faces.shape[0])
    return simplify_extracted(verts, faces, aabb, grid, k)[:3]


@torch.no_grad()
def export_mesh(model, path, level=0.005, gridSize=None, attributes=False, color="albedo", *, keep_largest=None,
                min_component_voxels=None, connectivity=6, report=None, simplify=None, **bake_kw):
    """extract_mesh + write_ply -> (number of vertices, number of faces).
    attributes=True: the vertex element becomes ATTRIBUTE_LAYOUT -- positions (bit-identical to the plain export), the baked
    shading normal, a display colour (vertex_colors), roughness, ambient occlusion, coverage, albedo and direct irradiance of
    bake.bake_points(model, *field_positions(...), **bake_kw); the face element is unchanged.
    keep_largest / min_component_voxels / connectivity: extract_mesh's component filter (floaters are neither written nor
    baked).  simplify=k: extract_mesh's face budget; the attributes are then baked at the simplified vertices."""
    verts, faces, normals = extract_mesh(model, level, gridSize, keep_largest=keep_largest,
                                         min_component_voxels=min_component_voxels, connectivity=connectivity, report=report,
                                         simplify=simplify)
    if not attributes:
        if bake_kw or color != "albedo":
            raise TypeError("color and the bake arguments need attributes=True")
        write_ply(path, verts, faces)
        return verts.shape[0], faces.shape[0]
    from . import bake
    grid = [int(g) for g in (model.gridSize if gridSize is None else gridSize)]
    pos, out_dir = field_positions(model.aabb, grid, verts, normals)
    b = bake.bake_points(model, pos.contiguous(), out_dir.contiguous(), **bake_kw)
    rgb = vertex_colors(b["albedo"], b.get("irradiance"), color)
    V = verts.shape[0]
    ao = b["ao"] if "ao" in b else torch.ones((V,), dtype=torch.float32, device=verts.device)
    irr = b["irradiance"] if "irradiance" in b else torch.zeros((V, 3), dtype=torch.float32, device=verts.device)
    cols = torch.cat([verts, b["normal"], b["roughness"][:, None], ao[:, None], b["coverage"][:, None], b["albedo"], irr],
                     dim=1).cpu().numpy()
    rgb = rgb.cpu().numpy()
    v = np.empty(V, dtype=ATTRIBUTE_LAYOUT)
    floats = [n for n, t in ATTRIBUTE_LAYOUT if t == "f4"]
    for k, name in enumerate(floats):
        v[name] = cols[:, k]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    f = np.empty(faces.shape[0], dtype=[("vertex_indices", "i4", (3,))])
    f["vertex_indices"] = faces.cpu().numpy()
    write_elements(path, [("vertex", v), ("face", f)])
    return V, faces.shape[0]
