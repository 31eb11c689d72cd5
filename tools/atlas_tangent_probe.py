"""What tests/test_gpu_atlas.py::test_export_textured_on_trained_field bounds by TAN_TOL, measured over several trainings (needs a
GPU).  The test trains its field with float atomics, so the field and its mesh differ from run to run; this tool trains
--runs times in one process and prints, per training, the face count, the largest per-component distance of tir_atlas_corners'
tangents from the float64 restatement (tests/atlas_reference.py), how many corners pass the bound, and the restatement's own
float32 - float64 distance on that mesh.

    python tools/atlas_tangent_probe.py [--runs 8] > profiles/atlas_tangent_trainings.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    import contextlib
    import io
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/atlas_tangent_probe.py needs a GPU")
    from tensoir_amd import mesh, ops
    from tests import atlas_reference as A
    from tests.train_sequence import reconstruct
    for run in range(args.runs):
        with contextlib.redirect_stdout(io.StringIO()):
            m = reconstruct().model
        verts, faces, normals = mesh.extract_mesh(m, simplify=3)
        F = faces.shape[0]
        cols, T = ops.atlas_layout(F, args.size)
        tan = ops.atlas_corners(verts, normals, faces, args.size, cols, T)[2].cpu().numpy()
        hv, hn, hf = verts.cpu().numpy(), normals.cpu().numpy(), faces.cpu().numpy()
        rtan = A.corners(hv, hn, hf, args.size, cols, T)[2]
        rtan32 = A.corners(hv, hn, hf, args.size, cols, T, dtype=np.float32)[2]
        err = np.abs(tan - rtan).max(1)
        print(f"training {run}: {F} faces, tangent max {err.max():.3e} against TAN_TOL {A.TAN_TOL:.1e}, {int((err > A.TAN_TOL).sum())} of "
              f"{3 * F} corners beyond it; restatement float32 - float64 {np.abs(rtan32 - rtan).max():.3e}", flush=True)


if __name__ == "__main__":
    main()
