"""tensoir_amd.regularisers without a GPU: the PyTorch fallback is the plain expression bit for bit, the model methods reproduce the
recorded reference values, the launcher rebinds the scripts' TVLoss, and tir_tv_* refuse bad calls before any device work."""
import ctypes as C
import importlib
import json
import os
import sys

import pytest
import torch

from tests import regulariser_reference as RR
from tests.helpers import golden_checkpoint, regulariser_trace, tv_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUP, OK = -1001, -1002, 0


# ---- fallback values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RR.SINGLE_SHAPES + RR.GRID_SHAPES)
def test_host_tensors_take_the_plain_expression_bit_for_bit(shape):
    from tensoir_amd import regularisers
    for channel_last in (True, False):
        x = RR.plane(shape, channel_last=channel_last).requires_grad_(True)
        y = x.detach().clone().requires_grad_(True)
        a, b = regularisers.TVLoss()(x), tv_loss(y)
        assert torch.equal(a, b)
        a.backward()
        b.backward()
        assert torch.equal(x.grad, y.grad)
        half = regularisers.TVLoss(0.5)
        assert half.TVLoss_weight == 0.5
        z = x.detach().clone().requires_grad_(True)
        c = half(z)
        c.backward()
        assert torch.equal(c, 0.5 * b.detach()) and torch.equal(z.grad, 0.5 * y.grad)
        # within rounding of the float64 restatement (fp32 sums of up to 1e5 terms: 1e-5 is far above them)
        assert abs(float(a.detach()) - RR.loss([x], [1.0])) <= 1e-5 * RR.loss([x], [1.0])


def test_unit_dimension_and_other_inputs_behave_as_the_plain_expression():
    from tensoir_amd import regularisers
    reg = regularisers.TVLoss()
    x = RR.plane((4, 5, 2))[:, :, :, :1]                              # [1, C, H, 1]: the W count is zero
    a, b = reg(x), tv_loss(x)
    assert not torch.isfinite(a) and torch.equal(a.isnan(), b.isnan()) and (bool(a.isnan()) or torch.equal(a, b))
    for other in (RR.plane((4, 5, 6)).double(), torch.cat([RR.plane((4, 5, 6)), RR.plane((4, 5, 6), seed=1)])):      # dtype, batch 2
        assert torch.equal(reg(other), tv_loss(other))
    assert not regularisers.on_kernel_path(RR.plane((4, 5, 6)))      # a host tensor never reaches the kernels


def test_model_methods_reproduce_the_recorded_reference_values(golden):
    import tensoir_amd
    from tensoir_amd import regularisers
    eh, ew = [int(v) for v in golden["scene/envmap_hw"]]
    m = tensoir_amd.model_from_checkpoint(golden_checkpoint(golden), "cpu", envmap_h=eh, envmap_w=ew)
    got = regulariser_trace(m, regularisers.TVLoss())
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "host_reference.json")))["regularisers"]
    for name in ("TV_loss_density", "TV_loss_app"):
        a = want["values"][name]
        assert abs(a - got["values"][name]) <= 1e-6 * max(1.0, abs(a)), name
    # and the plain callable gives the very same numbers on the host: the class falls back to it
    plain = regulariser_trace(m, tv_loss)
    assert all(plain["values"][k] == got["values"][k] for k in ("TV_loss_density", "TV_loss_app"))
    # a weight scales the model methods
    assert float(m.TV_loss_app(regularisers.TVLoss(0.5)).detach()) == pytest.approx(0.5 * got["values"]["TV_loss_app"], rel=1e-6)


# ---- rebinding --------------------------------------------------------------------------------------------------------------------
STUB_UTILS = "class TVLoss:\n    def __init__(self, TVLoss_weight=1):\n        self.TVLoss_weight = TVLoss_weight\n\n\nother = 3\n"


def test_launcher_rebinds_the_scripts_tvloss(tmp_path, monkeypatch):
    from tensoir_amd import regularisers, run
    root, elsewhere = tmp_path / "tree", tmp_path / "elsewhere"
    root.mkdir()
    elsewhere.mkdir()
    (root / "utils.py").write_text(STUB_UTILS)
    (root / "train_stub.py").write_text("from utils import *\n")
    (elsewhere / "utils.py").write_text(STUB_UTILS)
    names = ("utils", "train_stub")
    stale = {k: sys.modules[k] for k in names if k in sys.modules}
    for k in stale:
        monkeypatch.delitem(sys.modules, k)
    monkeypatch.setattr(sys, "path", [str(root)] + list(sys.path))
    monkeypatch.delenv("TENSOIR_TORCH_TV", raising=False)
    try:
        script, utils = importlib.import_module("train_stub"), importlib.import_module("utils")
        theirs = utils.TVLoss
        assert script.TVLoss is theirs
        monkeypatch.setenv("TENSOIR_TORCH_TV", "1")
        assert run._rebind_tv(str(root)) is False and utils.TVLoss is theirs and script.TVLoss is theirs
        monkeypatch.setenv("TENSOIR_TORCH_TV", "0")
        assert run._rebind_tv(str(elsewhere)) is False and utils.TVLoss is theirs            # this utils is not under that root
        assert run._rebind_tv(str(root)) is True
        assert utils.TVLoss is regularisers.TVLoss and script.TVLoss is regularisers.TVLoss and utils.other == 3 and script.other == 3
        assert script.TVLoss().TVLoss_weight == 1
        # a utils from outside the root is left alone
        for k in names:
            del sys.modules[k]
        monkeypatch.setattr(sys, "path", [str(elsewhere)] + [p for p in sys.path if p != str(root)])
        outside = importlib.import_module("utils")
        kept = outside.TVLoss
        assert run._rebind_tv(str(root)) is False and outside.TVLoss is kept
    finally:
        for k in names:
            sys.modules.pop(k, None)
        sys.modules.update(stale)


# ---- validation (no device work: every call below is refused, or empty) -----------------------------------------------------------
_KEEP = torch.zeros(64, dtype=torch.float32)      # a non-null, 16-byte aligned host address: never dereferenced
P = _KEEP.data_ptr()


@pytest.fixture(scope="module")
def lib():
    from tensoir_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def _ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def _f64(*v):
    return (C.c_double * len(v))(*v)


def test_entry_points_refuse_bad_calls_on_the_host(lib):
    from tensoir_amd import ops
    assert (ops.TV_MAX_PLANES, ops.TV_SHARE, ops.TV_FWD_GROUPS) == (8, 8192, 128)
    one, two = _i32(16), _i32(16, 48)
    good = dict(planes=_ptrs(P), C=one, H=_i32(8), W=_i32(8), coef=_f64(1.0), n=1, ws=P, sums=P, loss=P, g=P, grads=_ptrs(P))
    fwd = lambda **k: lib.tir_tv_fwd(*[{**good, **k}[a] for a in "planes C H W coef n ws sums loss".split()], None)
    bwd = lambda **k: lib.tir_tv_bwd(*[{**good, **k}[a] for a in "planes C H W coef n g grads".split()], None)
    wsp = lambda **k: lib.tir_tv_workspace(*[{**good, **k}[a] for a in "n C H W".split()])
    huge = dict(C=_i32(2 ** 20), H=_i32(2 ** 20), W=_i32(2 ** 20))       # 2^60 elements: beyond 2^31 workgroups of 8192
    for call in (fwd, bwd, wsp):
        assert call(n=-1) == ARG and call(n=9) == ARG
        assert call(n=0) == (1 if call is wsp else OK)
        assert call(n=0, C=None, H=None, W=None, planes=None, coef=None, ws=None, sums=None, loss=None, g=None, grads=None) == (1 if call is wsp else OK)
        assert call(C=None) == ARG and call(H=None) == ARG and call(W=None) == ARG
        assert call(C=_i32(0)) == ARG and call(C=_i32(-4)) == ARG
        assert call(H=_i32(1)) == ARG and call(W=_i32(1)) == ARG and call(H=_i32(-3)) == ARG and call(W=_i32(0)) == ARG
        assert call(n=2, C=two, H=_i32(8, 1), W=_i32(8, 8), planes=_ptrs(P, P), coef=_f64(1, 1), grads=_ptrs(P, P)) == ARG
        assert call(**huge) == UNSUP
        assert call(C=_i32(4), H=_i32(2 ** 15), W=_i32(2 ** 14)) == UNSUP                  # exactly 2^31 elements
    assert wsp() == 2 * 1 + 1 and wsp(C=_i32(48), H=_i32(37), W=_i32(41)) == 2 * 9 + 1           # 72816 floats: 9 shares
    assert wsp(n=2, C=two, H=_i32(2, 2), W=_i32(2, 2)) == 2 * 2 + 1
    assert wsp(C=_i32(48), H=_i32(150), W=_i32(150)) == 2 * 118 + 1                 # 1 080 000 floats: 118 shares of 9216, not 132 of 8192
    for missing in ("planes", "coef", "ws", "sums", "loss"):
        assert fwd(**{missing: None}) == ARG, missing
    for missing in ("planes", "coef", "g", "grads"):
        assert bwd(**{missing: None}) == ARG, missing
    assert fwd(planes=_ptrs(None)) == ARG and bwd(planes=_ptrs(None)) == ARG
    assert fwd(ws=None, **huge) == ARG and bwd(g=None, **huge) == ARG            # a missing pointer is reported before the size
    assert bwd(grads=_ptrs(None)) == OK                                          # no gradient wanted: nothing to do


def test_python_entry_points_refuse_what_the_kernels_cannot_take():
    from tensoir_amd import _lib, ops, regularisers
    x = RR.plane((4, 5, 6))
    with pytest.raises(_lib.TensoirHipError):
        ops.tv_forward([x], [1.0])                                               # host tensor: there is no CPU path in ops
    with pytest.raises(ValueError):
        regularisers.tv_planes([x], [1.0])
    with pytest.raises(ValueError):
        ops.tv_forward([], [])
    assert ops.is_channel_last(x) and not ops.is_channel_last(RR.plane((4, 5, 6), channel_last=False)) and not ops.is_channel_last(x.double())
