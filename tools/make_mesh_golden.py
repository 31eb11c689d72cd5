"""Record what scikit-image's marching cubes returns -> tests/golden/mesh_skimage.npz.

Run with an interpreter that has scikit-image (0.18.3 recorded) and numpy; torch is not needed:

    python tools/make_mesh_golden.py

Per case `<name>/`: vol (fp32, [gx][gy][gz]), level, spacing (fp32 [3]), scikit-image's verts / faces / normals as returned by
`marching_cubes(vol, level=level, spacing=[np.float32 x3])` -- the call `convert_sdf_samples_to_ply` makes, whose spacing is a
list of fp32 scalars -- and the dtype names of its four outputs.  Nothing here runs code of the reference project.
"""
import os
import sys

import numpy as np
import skimage
from skimage import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "mesh_skimage.npz")


def lattice(shape):
    """Coordinates in [-1, 1] per axis, fp32, indexing 'ij'."""
    ax = [np.linspace(-1, 1, n).astype(np.float32) for n in shape]
    return np.meshgrid(*ax, indexing="ij")


def blob(shape):
    """A smooth closed surface inside the lattice: an anisotropic ellipsoid with a cubic wobble (polynomial, fp32)."""
    x, y, z = lattice(shape)
    f = np.float32
    r = (x * x) / f(0.55) + (y * y) / f(0.4) + (z * z) / f(0.5)
    return (f(1) - r + f(0.25) * x * y * z + f(0.15) * x * x * y).astype(np.float32)


def cut_open(shape):
    """A sphere whose centre lies near a corner of the lattice: the lattice boundary cuts the surface open."""
    x, y, z = lattice(shape)
    f = np.float32
    return (f(1) - ((x - f(0.8)) ** 2 + (y + f(0.7)) ** 2 + z * z) / f(0.6)).astype(np.float32)


def on_level(shape):
    """Quantised values: many lattice points lie exactly on the level (0.5 in steps of 0.25)."""
    v = blob(shape)
    return (np.round(v * np.float32(4)) / np.float32(4)).astype(np.float32)


def cases():
    g = np.load(os.path.join(ROOT, "tests", "golden", "mask_maintenance.npz"))
    a = g["nomask/alpha"].astype(np.float32)
    yield "alpha", a, 0.005, np.float32(3.0) / np.array(a.shape, np.float32)
    yield "blob", blob((40, 48, 56)), 0.3, np.array([0.05, 0.04, 0.035], np.float32)
    yield "open", cut_open((24, 20, 28)), 0.0, np.array([0.1, 0.1, 0.1], np.float32)
    yield "onlevel", on_level((20, 24, 18)), 0.5, np.array([1.0, 1.0, 1.0], np.float32)


def main():
    rec = {"skimage_version": np.array(skimage.__version__)}
    names = []
    for name, vol, level, spacing in cases():
        level = float(np.float32(level))
        verts, faces, normals, values = measure.marching_cubes(vol, level=level, spacing=[np.float32(s) for s in spacing])
        names.append(name)
        p = name + "/"
        rec[p + "vol"] = vol
        rec[p + "level"] = np.array(level, np.float32)
        rec[p + "spacing"] = spacing
        rec[p + "verts"] = verts
        rec[p + "faces"] = faces
        rec[p + "normals"] = normals
        rec[p + "dtypes"] = np.array([verts.dtype.str, faces.dtype.str, normals.dtype.str, values.dtype.str])
        print(name, vol.shape, "verts", verts.shape, verts.dtype, "faces", faces.shape, faces.dtype, "normals", normals.dtype,
              "values", values.dtype)
    rec["cases"] = np.array(names)
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.exit(main())
