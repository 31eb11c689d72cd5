"""Record what the reference's own utils.rgb_ssim returns for the three-channel cases of tests/metrics_reference.py:

    TENSOIR_REFERENCE=/path/to/TensoIR python tools/make_golden_metrics.py

-> tests/golden/metrics_ssim.npz: "mean/<case>" (float64 scalar) for every three-channel case and "map/<case>" (float64 map) for
metrics_reference.MAP_CASES.  Recorded results only.  The reference is imported at run time, behind the launcher's stand-ins for
the third-party modules it imports (tensoir_amd/shims.py); it needs scipy.  No test runs this script."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ref = os.environ.get("TENSOIR_REFERENCE")
    if not ref or not os.path.isfile(os.path.join(ref, "utils.py")):
        raise SystemExit("set TENSOIR_REFERENCE to a TensoIR checkout")
    from tensoir_amd import shims
    from tests import metrics_reference as MR
    shims.install()
    sys.path.insert(0, ref)
    import utils
    assert os.path.realpath(utils.__file__).startswith(os.path.realpath(ref)), utils.__file__
    out = {}
    for name, a, b, kw in MR.cases():
        if a.shape[-1] != 3:
            continue
        kw = dict(kw)
        max_val = kw.pop("max_val", 1.0)
        out["mean/" + name] = np.float64(utils.rgb_ssim(a, b, max_val, **kw))
        if name in MR.MAP_CASES:
            out["map/" + name] = np.asarray(utils.rgb_ssim(a, b, max_val, return_map=True, **kw), dtype=np.float64)
        print(f"{name:14s} {a.shape} mean {out['mean/' + name]:.17g}")
    np.savez_compressed(MR.GOLDEN, **out)
    print("wrote", MR.GOLDEN, os.path.getsize(MR.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
