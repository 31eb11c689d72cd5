"""Mesh export of a trained field: scripts/export_mesh.py:15-24 -> utils.py:164-226 (convert_sdf_samples_to_ply), on the device.

    verts, faces, normals = extract_mesh(model)          # dense alpha lattice -> marching cubes (tir_dense_alpha, tir_mc_*)
    extract_mesh(model, keep_largest=1)                  # ... without the detached blobs ("floaters"): tir_ccl_* on the lattice
    export_mesh(model, "scene.ply")                      # + binary PLY, laid out as plyfile writes the reference's mesh
    export_mesh(model, "scene.ply", attributes=True)     # + per-vertex materials and direct lighting (tensoir_amd/bake.py)
    export_mesh(model, "scene.ply", simplify=3)          # a face budget: one vertex per 3 x 3 x 3 block of cells (tir_simplify_*)
    export_textured(model, "scene.glb", simplify=3)      # + a texture atlas baked at every texel, as a binary glTF (tir_atlas_*)
    export_mesh(model, "scene.ply", simplify_tolerance=0.5)   # the smallest mesh within half a cell of the full one
    distance((va, fa), (vb, fb))                         # how far two surfaces lie apart: Chamfer, Hausdorff (tir_distance.hip)
    distance(a, b, signed=True, thresholds=(0.5,), normals=True)   # + inflated or shrunk, F-score, normal consistency
    raycast((v, f), origins, dirs)                       # what a ray hits on the mesh, exactly (tir_ray_mesh)

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


SIMPLIFY_MAX = 8


def _check_simplify_options(simplify, simplify_tolerance, simplify_max=SIMPLIFY_MAX, measure_simplify=False):
    """-> (k or None, tolerance or None, the ks a tolerance search tries).  Raises before anything touches the device."""
    k = _check_simplify(simplify)
    if simplify_tolerance is None:
        if measure_simplify and k is None:
            raise ValueError("measure_simplify: needs simplify=k (simplify_tolerance measures every k it tries)")
        return k, None, ()
    if k is not None:
        raise ValueError("simplify and simplify_tolerance are mutually exclusive: a cluster size, or an error bound")
    if isinstance(simplify_tolerance, bool) or not isinstance(simplify_tolerance, (int, float, np.integer, np.floating)):
        raise ValueError(f"simplify_tolerance: expected a number of cells >= 0 or None, not {simplify_tolerance!r}")
    if not simplify_tolerance >= 0 or simplify_tolerance == float("inf"):
        raise ValueError(f"simplify_tolerance: must be a finite number of cells >= 0, not {simplify_tolerance}")
    if isinstance(simplify_max, bool) or not isinstance(simplify_max, (int, np.integer)) or simplify_max < 2:
        raise ValueError(f"simplify_max: expected an integer >= 2, not {simplify_max!r}")
    return None, float(simplify_tolerance), tuple(range(2, int(simplify_max) + 1))


def choose_simplify(measure, ks, tolerance):
    """The search policy of simplify_tolerance: try the ks in order, keep the last whose measure(k) (a float) is at most
    `tolerance`, stop at the first that is not (a NaN is not).  -> (the k kept or None, {k: measure(k)} of every k tried)."""
    chosen, tried = None, {}
    for k in ks:
        e = float(measure(k))
        tried[k] = e
        if not e <= tolerance:
            break
        chosen = k
    return chosen, tried


def distance_summary(d_vertices, d_samples):
    """The figures of one direction of distance() from distances that are already computed (tensors on any device, the CPU
    included): mean, rms and p95 (the 0.95 quantile, linear interpolation) over the area samples only, max over the samples
    and the vertices, n = the number of samples.  Sums in float64.  Without samples mean, rms and p95 are NaN; without any
    distance max is NaN too."""
    dv = torch.as_tensor(d_vertices).reshape(-1).to(torch.float64)
    ds = torch.as_tensor(d_samples).reshape(-1).to(torch.float64)
    n = ds.numel()
    nan = float("nan")
    both = torch.cat([dv, ds])
    p95 = nan
    if n:                                                     # (torch.quantile refuses more than 2^24 elements)
        pos = 0.95 * (n - 1)
        lo = int(pos)
        s = torch.sort(ds)[0][lo:lo + 2].tolist()
        p95 = s[0] + (s[-1] - s[0]) * (pos - lo)
    return {"mean": float(ds.sum() / n) if n else nan, "rms": float(torch.sqrt((ds * ds).sum() / n)) if n else nan,
            "max": float(both.max()) if both.numel() else nan, "p95": p95, "n": n}


def topology(verts, faces):
    """Whether the parity of ray crossings means inside (plain torch, on the device of the inputs).  Vertices are welded by
    position first (-0.0 as 0.0), so a mesh with three vertices of its own per face (what write_glb stores) is judged by its
    surface.  A face with a repeated welded vertex counts as "degenerate"; its self-edges are dropped.  -> {"closed": every
    directed edge (a, b) occurs as often as its reverse (b, a) -- the exact condition under which an odd number of crossings
    means inside; "boundary_edges": the directed edges without a partner, sum over edges of max(0, count(a, b) - count(b, a));
    "degenerate"}.  A face index outside [0, V) raises ValueError."""
    v = torch.as_tensor(verts).reshape(-1, 3)
    f = torch.as_tensor(faces).reshape(-1, 3).long().to(v.device)
    if f.numel() == 0:
        return {"closed": True, "boundary_edges": 0, "degenerate": 0}
    if int(f.min()) < 0 or int(f.max()) >= v.shape[0]:
        raise ValueError("topology: a face index lies outside [0, V)")
    uniq, inverse = torch.unique(v + 0.0, dim=0, return_inverse=True)
    w = inverse[f]                                            # [F, 3] welded indices
    a, b = w.reshape(-1), w.roll(-1, 1).reshape(-1)           # the directed edges (0, 1), (1, 2), (2, 0) of every face
    degenerate = int(((w[:, 0] == w[:, 1]) | (w[:, 1] == w[:, 2]) | (w[:, 2] == w[:, 0])).sum())
    keep = a != b
    a, b = a[keep], b[keep]
    n = uniq.shape[0]
    key, cnt = torch.unique(a * n + b, return_counts=True)
    rkey, rcnt = torch.unique(b * n + a, return_counts=True)  # (b, a) for every edge: how often the reverse of `rkey` occurs
    pos = torch.searchsorted(rkey, key).clamp(max=max(rkey.numel() - 1, 0))
    partner = torch.where(rkey[pos] == key, rcnt[pos], torch.zeros_like(cnt)) if key.numel() else cnt
    boundary = int((cnt - partner).clamp(min=0).sum())
    return {"closed": boundary == 0, "boundary_edges": boundary, "degenerate": degenerate}


def face_normals(verts, faces, index):
    """Unit fp64 normals (v1 - v0) x (v2 - v0) of faces `index` ([n] integer tensor); NaN for an index of -1 or a face without
    area."""
    idx = index.long()
    tri = verts.to(torch.float64)[faces.long()[idx.clamp(min=0)]]
    n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n = n / n.norm(dim=1, keepdim=True)
    return torch.where((idx >= 0)[:, None], n, torch.full_like(n, float("nan")))


@torch.no_grad()
def raycast(mesh, origins, dirs, grid=None, trange=None, mode="closest"):
    """Rays against a mesh: (verts [V, 3] f32, faces [F, 3] i32), origins and dirs [n, 3] f32 on the GPU (ops.ray_mesh: exact
    fp64 ray-triangle rule over ops.face_grid, bit-identical for every grid).  mode "closest" or "count".  -> {"t" [n] f32 (+inf
    on a miss, in units of |dir|), "face" [n] i32 (-1), "bary" [n, 2] f32 (weights of the face's second and third corner),
    "point" [n, 3] f32 = origin + t dir, "normal" [n, 3] f32 = the unit face normal (v1 - v0) x (v2 - v0), "count" [n] i32,
    "flags" [n] i32 (ops.RAY_GRAZED, ops.RAY_INVALID)}; bary, point and normal are NaN on a miss."""
    if mode not in ("closest", "count"):
        raise ValueError('raycast: mode "closest" or "count"')
    verts, faces = mesh
    t, face, bary, count, flags = ops.ray_mesh(origins, dirs, verts, faces, grid, mode=mode, trange=trange, bary=True, count=True,
                                               flags=True)
    hit = face >= 0
    nan = torch.full_like(origins.reshape(-1, 3), float("nan"))
    point = torch.where(hit[:, None], origins.reshape(-1, 3) + t[:, None] * dirs.reshape(-1, 3), nan)
    return {"t": t, "face": face, "bary": bary, "point": point, "normal": face_normals(verts, faces, face).float(), "count": count,
            "flags": flags}


def signed_summary(d_samples, inside, votes, grazed):
    """The signed figures of one direction from its samples' unsigned distances, and ops.mesh_inside's three outputs for them:
    signed_mean = the mean of -d for a sample inside the other mesh and +d outside (float64), inside_share, undecided = the
    samples whose three votes are not unanimous, grazed = the samples one of whose rays passed through an edge or a vertex."""
    ds = torch.as_tensor(d_samples).reshape(-1).to(torch.float64)
    inside, votes, grazed = (torch.as_tensor(x).reshape(-1) for x in (inside, votes, grazed))
    n = ds.numel()
    nan = float("nan")
    sd = torch.where(inside.bool(), -ds, ds)
    return {"signed_mean": float(sd.sum() / n) if n else nan, "inside_share": float(inside.bool().sum()) / n if n else nan,
            "undecided": int(((votes == 1) | (votes == 2)).sum()), "grazed": int(grazed.bool().sum())}


def normal_summary(n_own, n_near):
    """normal_consistency = the mean |n . n'| over the samples (Occupancy Networks), flipped_share = the share with n . n' < 0;
    n, n' [k, 3] unit normals, sums in float64."""
    dot = (torch.as_tensor(n_own).to(torch.float64) * torch.as_tensor(n_near).to(torch.float64)).sum(1)
    k = dot.numel()
    nan = float("nan")
    return {"normal_consistency": float(dot.abs().sum() / k) if k else nan, "flipped_share": float((dot < 0).sum()) / k if k else nan}


def fscore_summary(d_a, d_b, thresholds):
    """Per threshold: precision = the share of a's sample distances <= it, recall = the share of b's, fscore = 2 P R / (P + R)
    (0 when both are 0); a is the prediction, b the ground truth."""
    da, db = torch.as_tensor(d_a).reshape(-1), torch.as_tensor(d_b).reshape(-1)
    out = []
    for tau in thresholds:
        p = float((da <= tau).sum()) / da.numel() if da.numel() else 0.0
        r = float((db <= tau).sum()) / db.numel() if db.numel() else 0.0
        out.append({"threshold": float(tau), "precision": p, "recall": r, "fscore": 2.0 * p * r / (p + r) if p + r > 0 else 0.0})
    return out


def _one_way(src, dst, grid, samples, seed, signed=False, normals=False):
    v, f = src
    used = torch.unique(f.reshape(-1).long())                 # the vertices a face refers to, ascending
    query = v[used]
    pts = own = None
    if samples > 0:
        pts, own = ops.sample_surface(v, f, samples, seed)
        query = torch.cat([query, pts])
    d, near = ops.point_mesh_distance(query, dst[0], dst[1], grid)
    ds = d[used.numel():]
    out = distance_summary(d[:used.numel()], ds)
    if signed:
        empty = v.new_zeros((0, 3))
        out.update(signed_summary(ds, *ops.mesh_inside(empty if pts is None else pts, dst[0], dst[1], grid)))
    if normals:
        none = near[:0]
        out.update(normal_summary(face_normals(v, f, none if own is None else own), face_normals(dst[0], dst[1], near[used.numel():])))
    return out, ds


def _check_distance_options(samples, signed, thresholds, normals, allow_open):
    samples = int(samples)
    if samples < 0:
        raise ValueError("distance: samples >= 0")
    if thresholds is not None:
        thresholds = tuple(float(t) for t in ([thresholds] if isinstance(thresholds, (int, float)) else thresholds))
        if not thresholds or any(not t >= 0.0 for t in thresholds):
            raise ValueError("distance: thresholds is a non-empty sequence of distances >= 0")
    for name, flag in (("signed", signed), ("normals", normals), ("allow_open", allow_open)):
        if not isinstance(flag, bool):
            raise ValueError(f"distance: {name} is True or False")
    if allow_open and not signed:
        raise ValueError("distance: allow_open belongs to signed=True")
    return samples, thresholds


@torch.no_grad()
def distance(a, b, samples=262144, seed=0, *, signed=False, thresholds=None, normals=False, allow_open=False):
    """How far two surfaces lie apart.  a, b: (verts [V, 3] f32, faces [F, 3] i32) on the GPU -> {"a_to_b", "b_to_a": {mean, rms,
    max, p95, n}, "chamfer": a_to_b.mean + b_to_a.mean, "hausdorff": max(a_to_b.max, b_to_a.max)}, in the coordinates of the
    inputs.  A direction's queries are the vertices its mesh's faces refer to, followed by `samples` area-weighted stratified
    samples of its surface (ops.sample_surface with `seed`, the same for both directions); each is measured exactly against the
    other mesh (ops.point_mesh_distance over ops.face_grid).  mean, rms and p95 are taken over the samples, max over both
    (distance_summary).  The same inputs give the same bits on every run.
    signed=True: each direction gains signed_mean, inside_share, undecided and grazed (signed_summary): a sample inside the other
    mesh (ops.mesh_inside: the parity of three exact rays) counts with -distance; the magnitudes are the same bits.  Parity needs
    a closed surface: a destination mesh that topology() does not find closed raises ValueError with its boundary-edge count,
    unless allow_open=True.  thresholds=(tau, ...): "fscore" = fscore_summary over the samples' distances (a = prediction, b =
    ground truth).  normals=True: each direction gains normal_consistency and flipped_share (normal_summary) between the fp64
    normal of each sample's own face and that of its nearest face on the other mesh.  With none of the three the result and
    its bits are what they were and no ray is cast."""
    samples, thresholds = _check_distance_options(samples, signed, thresholds, normals, allow_open)
    (va, fa), (vb, fb) = a, b
    if signed and not allow_open:
        for name, (v, f) in (("a", a), ("b", b)):
            topo = topology(v, f)
            if not topo["closed"]:
                raise ValueError(f"distance: signed=True needs closed surfaces, mesh {name} has {topo['boundary_edges']} boundary edges "
                                 "(allow_open=True takes the parity as it comes)")
    ga, gb = ops.face_grid(va, fa), ops.face_grid(vb, fb)
    ab, da = _one_way((va, fa), (vb, fb), gb, samples, seed, signed, normals)
    ba, db = _one_way((vb, fb), (va, fa), ga, samples, seed, signed, normals)
    out = {"a_to_b": ab, "b_to_a": ba, "chamfer": ab["mean"] + ba["mean"], "hausdorff": max(ab["max"], ba["max"])}
    if thresholds is not None:
        out["fscore"] = fscore_summary(da, db, thresholds)
    return out


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
                 report=None, simplify=None, simplify_tolerance=None, simplify_max=SIMPLIFY_MAX, measure_simplify=False):
    """getDenseAlpha(gridSize) (default: the model's gridSize) -> marching cubes at `level` in the reference's coordinates
    (module docstring).  -> (verts [V, 3] f32, faces [F, 3] i32 outward, normals [V, 3] f32), on the model's device.
    keep_largest / min_component_voxels (select_components): the lattice's components under `connectivity` that fail the
    selection are set to 0 before marching cubes.  With connectivity 6 that removes whole closed surfaces and leaves every kept
    vertex bit-identical.  Needs level >= 0.  With both None no labelling kernel runs.
    simplify=k (an integer >= 2): the mesh is then reduced by quadric vertex clustering over blocks of k x k x k marching-cubes
    cells (simplify_extracted; the component filter runs first, on the lattice); the normals are the clusters' summed face
    normals in index space.  report (a dict) receives "full" = (vertices, faces) before the reduction.  With None no
    simplification kernel runs.
    simplify_tolerance=t (mutually exclusive with simplify): t is in marching-cubes cells, a distance divided by the smallest
    component of reference_spacing.  k = 2, 3, ..., simplify_max are tried in turn; the last k whose Hausdorff distance to the
    full-resolution mesh (after the component filter; distance(simplified, full)) is at most t is taken, the search stops at the
    first k that fails (choose_simplify), and when k = 2 already fails the full mesh is returned.  report receives "simplify"
    (the k taken, or None) and "simplify_error" = {k: distance's dict plus "cell", the length of one cell} of every k tried.
    measure_simplify=True with simplify=k: report["simplify_error"] = that dict for k (a = the simplified mesh, b = the full one).
    With neither option no distance kernel runs."""
    filtering = _check_component_options(keep_largest, min_component_voxels, connectivity)
    k, tolerance, ks = _check_simplify_options(simplify, simplify_tolerance, simplify_max, measure_simplify)
    grid = _model_grid(model, gridSize)
    alpha, _ = ops.dense_alpha(model.packed_field(), grid, float(model.stepSize))   # getDenseAlpha's alpha, no xyz lattice
    if filtering:
        alpha, table, kept = _filtered_alpha(alpha, level, keep_largest, min_component_voxels, connectivity)
        if report is not None:
            report.update(table=table, kept=kept)
    aabb = model.aabb.detach().to("cpu", torch.float32)
    verts, faces, normals = ops.marching_cubes(alpha, level, reference_spacing(aabb, grid), aabb[0].tolist())
    if k is None and tolerance is None:
        return verts, faces, normals
    if report is not None:
        report["full"] = (verts.shape[0], faces.shape[0])
    cell = min(reference_spacing(aabb, grid))

    def measured(kk):
        out = simplify_extracted(verts, faces, aabb, grid, kk)[:3]
        err = distance((out[0], out[1]), (verts, faces))
        err["cell"] = cell
        return out, err

    if tolerance is None:
        if not measure_simplify:
            return simplify_extracted(verts, faces, aabb, grid, k)[:3]
        out, err = measured(k)
        if report is not None:
            report["simplify_error"] = err
        return out
    meshes, errors = {}, {}

    def measure(kk):
        meshes[kk], errors[kk] = measured(kk)
        return errors[kk]["hausdorff"] / cell

    taken, _ = choose_simplify(measure, ks, tolerance)
    if report is not None:
        report.update(simplify=taken, simplify_error=errors)
    return (verts, faces, normals) if taken is None else meshes[taken]


@torch.no_grad()
def export_mesh(model, path, level=0.005, gridSize=None, attributes=False, color="albedo", *, keep_largest=None,
                min_component_voxels=None, connectivity=6, report=None, simplify=None, simplify_tolerance=None,
                simplify_max=SIMPLIFY_MAX, measure_simplify=False, **bake_kw):
    """extract_mesh + write_ply -> (number of vertices, number of faces).
    attributes=True: the vertex element becomes ATTRIBUTE_LAYOUT -- positions (bit-identical to the plain export), the baked
    shading normal, a display colour (vertex_colors), roughness, ambient occlusion, coverage, albedo and direct irradiance of
    bake.bake_points(model, *field_positions(...), **bake_kw); the face element is unchanged.
    keep_largest / min_component_voxels / connectivity: extract_mesh's component filter (floaters are neither written nor
    baked).  simplify=k: extract_mesh's face budget; the attributes are then baked at the simplified vertices.
    simplify_tolerance / simplify_max / measure_simplify: extract_mesh's error-bounded face budget and its report."""
    verts, faces, normals = extract_mesh(model, level, gridSize, keep_largest=keep_largest,
                                         min_component_voxels=min_component_voxels, connectivity=connectivity, report=report,
                                         simplify=simplify, simplify_tolerance=simplify_tolerance, simplify_max=simplify_max,
                                         measure_simplify=measure_simplify)
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


# ---- textured export: a per-triangle atlas baked on the device, written as a binary glTF -----------------------------
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"
IMAGE_NAMES = ("base", "orm", "normal")          # base colour (sRGB), occlusion / roughness / metallic (linear), tangent-space normal


def _png_chunk(kind, data):
    import struct
    import zlib
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(rgba_uint8, compress_level=6):
    """[H, W, 4] uint8 -> the bytes of an 8-bit RGBA PNG: one IDAT chunk, every scanline with filter type 0."""
    import struct
    import zlib
    a = np.asarray(rgba_uint8.cpu() if torch.is_tensor(rgba_uint8) else rgba_uint8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: expected [H, W, 4] uint8, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    raw = np.zeros((h, 1 + 4 * w), np.uint8)
    raw[:, 1:] = a.reshape(h, 4 * w)
    return (_PNG_MAGIC + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
            _png_chunk(b"IDAT", zlib.compress(raw.tobytes(), int(compress_level))) + _png_chunk(b"IEND", b""))


def read_png(data):
    """The inverse of write_png (8-bit RGBA, no interlace, filter type 0 on every scanline) -> [H, W, 4] uint8."""
    import struct
    import zlib
    if data[:8] != _PNG_MAGIC:
        raise ValueError("read_png: not a PNG")
    pos, head, idat = 8, None, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError(f"read_png: bad CRC in chunk {kind!r}")
        pos += 12 + n
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if head is None or head[2:] != (8, 6, 0, 0, 0):
        raise ValueError("read_png: only 8-bit RGBA without interlace is supported")
    w, h = head[:2]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, 1 + 4 * w)
    if raw[:, 0].any():
        raise ValueError("read_png: only filter type 0 is supported")
    return raw[:, 1:].reshape(h, w, 4).copy()


_GLB_MAGIC, _GLB_JSON, _GLB_BIN = 0x46546C67, 0x4E4F534A, 0x004E4942
_GLTF_FLOAT, _GLTF_ARRAY_BUFFER, _GLTF_LINEAR, _GLTF_CLAMP, _GLTF_TRIANGLES = 5126, 34962, 9729, 33071, 4
_GLB_ATTRIBUTES = (("POSITION", "VEC3", 3), ("NORMAL", "VEC3", 3), ("TANGENT", "VEC4", 4), ("TEXCOORD_0", "VEC2", 2))


def write_glb(path, pos, nrm, tan, uv, images, extras=None, occlusion=True, compress_level=6):
    """A single-file binary glTF 2.0: one non-indexed TRIANGLES primitive with POSITION [3F, 3], NORMAL [3F, 3], TANGENT [3F, 4]
    and TEXCOORD_0 [3F, 2] (float32), one metallic-roughness material whose textures are the PNG-encoded `images`
    {"base", "orm", "normal": [S, S, 4] uint8}, embedded in the one buffer.  occlusion: the material's occlusionTexture points
    at the ORM image (its red channel) -- leave it out when no lighting was baked.  One sampler, LINEAR / LINEAR without
    mip-maps (they would bleed across the atlas cells) and CLAMP_TO_EDGE.  extras goes to the root's extras.tensoir_amd.
    One JSON chunk padded with spaces and one BIN chunk padded with zeros, every buffer view 4-byte aligned."""
    import json
    import struct
    host = lambda t, k: np.ascontiguousarray(np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, np.float32).reshape(-1, k))
    arrays = [host(t, k) for t, (_, _, k) in zip((pos, nrm, tan, uv), _GLB_ATTRIBUTES)]
    n = arrays[0].shape[0]
    if n % 3 or any(a.shape[0] != n for a in arrays):
        raise ValueError("write_glb: the attributes take one row per triangle corner")
    if sorted(images) != sorted(IMAGE_NAMES):
        raise ValueError(f"write_glb: images takes {IMAGE_NAMES}")
    blob, views = bytearray(), []

    def add_view(data, target=None):
        blob.extend(b"\0" * (-len(blob) % 4))
        view = {"buffer": 0, "byteOffset": len(blob), "byteLength": len(data)}
        if target is not None:
            view["target"] = target
        views.append(view)
        blob.extend(data)
        return len(views) - 1

    accessors, attributes = [], {}
    for a, (name, kind, _) in zip(arrays, _GLB_ATTRIBUTES):
        acc = {"bufferView": add_view(a.astype("<f4").tobytes(), _GLTF_ARRAY_BUFFER), "componentType": _GLTF_FLOAT, "count": n,
               "type": kind}
        if name == "POSITION":
            acc["min"] = [float(x) for x in a.min(0)] if n else [0.0] * 3
            acc["max"] = [float(x) for x in a.max(0)] if n else [0.0] * 3
        attributes[name] = len(accessors)
        accessors.append(acc)
    gl_images = [{"name": name, "mimeType": "image/png", "bufferView": add_view(write_png(images[name], compress_level))}
                 for name in IMAGE_NAMES]
    material = {"name": "baked", "pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicRoughnessTexture": {"index": 1},
                                                          "metallicFactor": 1.0, "roughnessFactor": 1.0},
                "normalTexture": {"index": 2}}
    if occlusion:
        material["occlusionTexture"] = {"index": 1}
    doc = {"asset": {"version": "2.0", "generator": "tensoir_amd"}, "scene": 0, "scenes": [{"nodes": [0]}],
           "nodes": [{"mesh": 0}],
           "meshes": [{"primitives": [{"attributes": attributes, "material": 0, "mode": _GLTF_TRIANGLES}]}],
           "materials": [material],
           "textures": [{"sampler": 0, "source": i} for i in range(3)],
           "images": gl_images,
           "samplers": [{"magFilter": _GLTF_LINEAR, "minFilter": _GLTF_LINEAR, "wrapS": _GLTF_CLAMP, "wrapT": _GLTF_CLAMP}],
           "accessors": accessors, "bufferViews": views, "buffers": [{"byteLength": len(blob)}],
           "extras": {"tensoir_amd": dict(extras or {})}}
    text = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    text += b" " * (-len(text) % 4)
    body = bytes(blob) + b"\0" * (-len(blob) % 4)
    total = 12 + 8 + len(text) + 8 + len(body)
    with open(path, "wb") as f:
        f.write(struct.pack("<III", _GLB_MAGIC, 2, total))
        f.write(struct.pack("<II", len(text), _GLB_JSON) + text)
        f.write(struct.pack("<II", len(body), _GLB_BIN) + body)


def read_glb(path):
    """The inverse of write_glb -> {"pos", "nrm", "tan", "uv": float32 arrays, "images": {"base", "orm", "normal": [S, S, 4]
    uint8}, "json": the document}."""
    import json
    import struct
    data = open(path, "rb").read()
    magic, version, total = struct.unpack("<III", data[:12])
    if magic != _GLB_MAGIC or version != 2 or total != len(data):
        raise ValueError("read_glb: not a binary glTF 2.0 file of the length its header states")
    n_json, kind = struct.unpack("<II", data[12:20])
    if kind != _GLB_JSON:
        raise ValueError("read_glb: the first chunk must be JSON")
    doc = json.loads(data[20:20 + n_json].decode("utf-8"))
    n_bin, kind = struct.unpack("<II", data[20 + n_json:28 + n_json])
    if kind != _GLB_BIN or 28 + n_json + n_bin != total:
        raise ValueError("read_glb: expected one BIN chunk after the JSON chunk")
    blob = data[28 + n_json:]

    def view(i):
        v = doc["bufferViews"][i]
        return blob[v.get("byteOffset", 0):v.get("byteOffset", 0) + v["byteLength"]]

    prim = doc["meshes"][0]["primitives"][0]
    out = {"json": doc, "images": {}}
    for key, (name, _, k) in zip(("pos", "nrm", "tan", "uv"), _GLB_ATTRIBUTES):
        acc = doc["accessors"][prim["attributes"][name]]
        out[key] = np.frombuffer(view(acc["bufferView"]), "<f4", count=acc["count"] * k).reshape(-1, k).astype(np.float32)
    for img in doc["images"]:
        out["images"][img["name"]] = read_png(view(img["bufferView"]))
    return out


def _check_texture_options(size, color, bake_kw):
    """Raises before anything touches the device."""
    import numbers
    if isinstance(size, bool) or not isinstance(size, numbers.Integral) or not ops.ATLAS_MIN_T <= size <= ops.ATLAS_MAX_SIZE:
        raise ValueError(f"size: expected an integer in {ops.ATLAS_MIN_T} .. {ops.ATLAS_MAX_SIZE}, not {size!r}")
    if color not in ("albedo", "diffuse"):
        raise ValueError(f"color: 'albedo' or 'diffuse', not {color!r}")
    if color == "diffuse" and not bake_kw.get("lighting", True):
        raise ValueError('color="diffuse" needs the baked irradiance (lighting=True)')


@torch.no_grad()
def bake_atlas(model, verts, faces, normals, grid, size=2048, color="albedo", edits=None, **bake_kw):
    """A texture atlas of the mesh (verts, faces, normals) as extract_mesh returns it -- file coordinates, index-space normals --
    with one texel sample of the field per owned texel.  Layout (ops.atlas_layout; include/tensoir_hip.h, tir_atlas_*): no chart
    solver, faces 2c and 2c+1 share the square cell c of T x T texels, T = size // ceil(sqrt(ceil(F / 2))).
    tir_atlas_texels interpolates position and normal at every texel centre in the mesh's own spaces, field_positions maps
    them to the field, bake.bake_points(**bake_kw) bakes them, tir_atlas_pack writes the images.
    -> {"pos" [3F, 3], "nrm" [3F, 3], "tan" [3F, 4], "uv" [3F, 2]: the unwelded mesh (float32), "base", "orm", "normal":
    [size, size, 4] uint8 images, "cols", "T"}, tensors on verts' device.  base is sRGB of the albedo, or of the Lambertian
    radiance under the baked light (color="diffuse"); orm holds occlusion (255 with lighting=False), roughness, 0; normal is the
    baked shading normal in the frame (tangent, cross(n, tangent), n) of the interpolated mesh normal n.
    edits (a materials.EditList or a list of MaterialEdit; None: no kernel is added, the images keep their bits):
    materials.apply runs on the bake's albedo and roughness at its surface positions before the images are packed.  The base
    colour then encodes the edited `base` (glTF: the viewer forms the diffuse part from base and metallic; color="diffuse" lights
    base (1 - metal)), G of orm the edited roughness and B of orm the metallic value (tir_atlas_metal)."""
    from . import bake, materials
    _check_texture_options(size, color, bake_kw)
    edits = materials.as_edit_list(edits)
    F = faces.shape[0]
    cols, T = ops.atlas_layout(F, size)
    pos, nrm, tan, uv = ops.atlas_corners(verts, normals, faces, size, cols, T)
    point, outward, _ = ops.atlas_texels(verts, normals, faces, size, cols, T)
    p, d = field_positions(model.aabb, grid, point, outward)
    b = bake.bake_points(model, p.contiguous(), d.contiguous(), **bake_kw)
    albedo, roughness, metal = b["albedo"], b["roughness"], None
    if edits is not None and len(edits) > 0:
        # the asset carries no Fresnel texture (a glTF viewer takes 0.04 for dielectrics): the row's F0 is that constant here
        e = materials.apply(b["surface"], albedo, roughness, torch.full_like(albedo, 0.04), edits)
        albedo, roughness, metal = e["albedo" if color == "diffuse" else "base"], e["roughness"], e["metal"]
    base, orm, normal = ops.atlas_pack(verts, normals, faces, size, cols, T, albedo, roughness, b["normal"], b["coverage"],
                                       irradiance=b["irradiance"] if color == "diffuse" else None, ao=b.get("ao"))
    if metal is not None and F > 0:
        ops.atlas_metal(orm, cols, T, F, metal)
    return {"pos": pos, "nrm": nrm, "tan": tan, "uv": uv, "base": base, "orm": orm, "normal": normal, "cols": cols, "T": T}


@torch.no_grad()
def export_textured(model, path, level=0.005, gridSize=None, size=2048, color="albedo", *, keep_largest=None,
                    min_component_voxels=None, connectivity=6, simplify=None, report=None, compress_level=6,
                    simplify_tolerance=None, simplify_max=SIMPLIFY_MAX, measure_simplify=False, edits=None, **bake_kw):
    """extract_mesh + bake_atlas + write_glb: the mesh as a single-file binary glTF 2.0 with base-colour, occlusion / roughness /
    metallic and tangent-space normal textures -> (number of triangle corners = 3 F, number of faces).
    Positions are the PLY export's coordinates, the reference's voxel-size quirk included (module docstring), and the file's
    axes are the field's: there is NO axis conversion to glTF's +Y-up convention.  The mesh is unwelded (three vertices per
    face, no index buffer).  keep_largest / min_component_voxels / connectivity / simplify: extract_mesh's options; the texture
    keeps the field's detail at every texel whatever the face budget.  compress_level: zlib's, for the PNG images.
    simplify_tolerance / simplify_max / measure_simplify: extract_mesh's error-bounded face budget and its report.
    The root's extras.tensoir_amd records size, cols, T, faces, level, simplify (the k taken), color and light_idx.
    edits: bake_atlas's material edits; the list's JSON is recorded as extras.tensoir_amd.edits.  An asset with
    metal is for a glTF viewer: raster.relight_glb / relight_mesh keep their scalar fresnel and do not read orm's B channel."""
    from . import materials
    edits = materials.as_edit_list(edits)
    _check_component_options(keep_largest, min_component_voxels, connectivity)
    _check_simplify_options(simplify, simplify_tolerance, simplify_max, measure_simplify)
    _check_texture_options(size, color, bake_kw)
    if isinstance(compress_level, bool) or not isinstance(compress_level, (int, np.integer)) or not 0 <= compress_level <= 9:
        raise ValueError(f"compress_level: expected an integer in 0 .. 9, not {compress_level!r}")
    grid = _model_grid(model, gridSize)
    report = {} if report is None else report
    verts, faces, normals = extract_mesh(model, level, gridSize, keep_largest=keep_largest,
                                         min_component_voxels=min_component_voxels, connectivity=connectivity, report=report,
                                         simplify=simplify, simplify_tolerance=simplify_tolerance, simplify_max=simplify_max,
                                         measure_simplify=measure_simplify)
    if simplify_tolerance is not None:
        simplify = report["simplify"]
    a = bake_atlas(model, verts, faces, normals, grid, size, color, edits=edits, **bake_kw)
    F = faces.shape[0]
    light = bake_kw.get("light_idx", 0)
    extras = {"size": int(size), "cols": a["cols"], "T": a["T"], "faces": F, "level": float(level),
              "simplify": None if simplify is None else int(simplify), "color": color,
              "light_idx": int(light) if not torch.is_tensor(light) else None}
    if edits is not None:
        extras["edits"] = edits.to_json()
    write_glb(path, a["pos"], a["nrm"], a["tan"], a["uv"], {k: a[k].cpu().numpy() for k in IMAGE_NAMES}, extras,
              occlusion=bool(bake_kw.get("lighting", True)), compress_level=int(compress_level))
    return 3 * F, F


@torch.no_grad()
def export_environment(model, path, H=256, W=512, light=0):
    """The illumination the model has recovered as a Radiance picture: model.get_light_rgbs at the H x W cell-centre directions
    of relight.Environment_Light (row i at phi = pi/2 - (i + 0.5) pi/H, column j at theta = pi - (j + 0.5) 2 pi/W, direction
    (cos theta cos phi, sin theta cos phi, sin phi)), row `light` of the result, written with hdr.write_hdr.  Read back and
    handed to Environment_Light(hdr_maps=...) or raster.relight_glb, the file therefore means the same illumination in world
    space.  light_kind 'sg' and 'pixel'; 'gt' passes the data set's probe through (and raises the model's own error without
    one).  -> the [H, W, 3] float32 array that was written (before the RGBE rounding)."""
    from .hdr import write_hdr
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("export_environment: H, W >= 1")
    lat, lng = np.pi / H, 2 * np.pi / W
    phi, theta = torch.meshgrid([torch.linspace(np.pi / 2 - 0.5 * lat, -np.pi / 2 + 0.5 * lat, H),
                                 torch.linspace(np.pi - 0.5 * lng, -np.pi + 0.5 * lng, W)], indexing="ij")
    dirs = torch.stack([torch.cos(theta) * torch.cos(phi), torch.sin(theta) * torch.cos(phi), torch.sin(phi)], dim=-1).view(-1, 3)
    rgbs = model.get_light_rgbs(dirs, device=model.aabb.device)
    if not 0 <= int(light) < rgbs.shape[0]:
        raise ValueError(f"export_environment: light outside 0 .. {rgbs.shape[0] - 1}")
    rgb = rgbs[int(light)].detach().reshape(H, W, 3).to("cpu", torch.float32).numpy()
    write_hdr(path, rgb)
    return rgb
