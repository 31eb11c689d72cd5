"""torch-tensor front end of the C ABI: argument checking, output allocation, stream plumbing.

PyTorch is used for device memory and streams only; every arithmetic step of the hot path runs in
libtensoir_hip.so.  All functions require CUDA(HIP) tensors and raise otherwise -- no fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import TirEnvSG, TirField, TirFieldHalf, TirMlp, check, lib

_K = _lib.CONST      # the #define constants of include/tensoir_hip.h
MAP_STRIDE = _K["TIR_MAP_STRIDE"]

# Optional instrumentation used by bench.py: when STATS is a dict, the march wrappers accumulate the
# number of gathered density samples per kernel (device-side counter, read back by the caller), and
# when TIMING is a list every C call is bracketed by events on the launch stream.
STATS = None
TIMING = None

# Launch options (performance only; results are the same either way).  The library itself keeps no settable state and reads no
# environment variable: the options travel in the descriptors / arguments of each call, and THIS module is where
# their defaults come from -- the environment of the embedding process, read once at import:
#   TENSOIR_LDS_LINES=0   secondary march without the LDS-staged line factors        -> TirField.tune_lds_lines = 2
#   TIR_XCD=1             contiguous per-XCD work ranges in the gathers / the march   -> TirField.tune_xcd_order = 1
#   TENSOIR_MLP_GRID=n    persistent workgroups of a decoder launch (default 256)     -> TirMlp.tune_grid = n
#   TIR_PAIR_ORDER=m      point-major secondary pair list (default direction-major)   -> tir_shade_setup_compact(pair_order = 2)
#   TENSOIR_DENSE_SIGMA=0 inference secondary marches without the dense density volume -> TirField.dense_sigma = NULL
#   TENSOIR_DENSE_SIGMA_MAX_MB=n   largest dense density volume that is built (default 1024; 300^3 needs 108 MB, 400^3 257 MB)
#   TENSOIR_DENSE_APP=0   inference indirect-light records without the dense appearance volume -> TirField.dense_app = NULL
#   TENSOIR_DENSE_APP_MAX_MB=n     largest dense appearance volume that is built (default 4096; 300^3 needs 1.73 GB; 4 GiB is
#                                  the kernels' limit)
# (the dense volumes are the options that are not bit-neutral: the march's density feature differs in its last fp32 bits, the
#  f16 tier's appearance features by fp16 roundings -- rgb_with_brdf_map within the precision policy's own limit)
TUNE = {
    "dense_app": 0 if os.environ.get("TENSOIR_DENSE_APP", "1") == "0" else 1,
    "dense_app_max_mb": max(0, int(os.environ.get("TENSOIR_DENSE_APP_MAX_MB", "4096") or 0)),
    "lds_lines": 2 if os.environ.get("TENSOIR_LDS_LINES", "1") == "0" else 0,
    "xcd_order": 1 if os.environ.get("TIR_XCD", "0") == "1" else 0,
    "dense_sigma": 0 if os.environ.get("TENSOIR_DENSE_SIGMA", "1") == "0" else 1,
    "dense_sigma_max_mb": max(0, int(os.environ.get("TENSOIR_DENSE_SIGMA_MAX_MB", "1024") or 0)),
    "mlp_grid": max(0, int(os.environ.get("TENSOIR_MLP_GRID", "0") or 0)),
    "pair_order": 2 if os.environ.get("TIR_PAIR_ORDER", "d")[:1] == "m" else 0,
    # TENSOIR_WGRAD_BLOCKS=n: workgroups of the fused weight-gradient launch (0 = 256: each fills a CU).  It runs on the leaf
    # stream beside the scatter / decoder-backward chain; measured (tools/train_bench.py, same box): 256 -> 4.1-4.3 ms per step,
    # 128 -> 4.6, 96 -> 4.6, 64 -> 5.2, 48 -> 7.0: with fewer workgroups the scatter kernels get faster (1.14 -> 0.92 ms) but
    # the leaf launch becomes the critical path
    "wgrad_blocks": max(0, int(os.environ.get("TENSOIR_WGRAD_BLOCKS", "0") or 0)),
}
# TENSOIR_MLP_AUXTAB=0: decoders whose aux input comes through an index map (the radiance decoder's view direction: one per ray
# or per light direction) run the full 150-input layer 1 instead of the aux-table variant (tir_mlp_aux_table + 9 k-blocks)
AUX_TABLE = os.environ.get("TENSOIR_MLP_AUXTAB", "1") != "0"
AUX_TABLE_MULTI = os.environ.get("TENSOIR_MLP_AUXTAB_MULTI", "0") == "1"


def mlp_aux_table(m: "PackedMlp", aux):
    """T[a][unit] = b0 + W0[:, aux columns] x(aux_a) for every row of `aux` [n_aux, 3] -> [n_aux, 128] fp32 (tir_mlp_aux_table):
    the start values of the layer-1 accumulators in the aux-table decoder launches."""
    aux = f32(aux, "aux", 3)
    table = torch.empty((aux.shape[0], 128), dtype=torch.float32, device=aux.device)
    _call("tir_mlp_aux_table", C.byref(m.desc), _ptr(aux), aux.shape[0], _ptr(table), _stream())
    return table


# While a HIP graph is being captured (GraphedRenderer._capture sets this to a list it keeps for the graph's lifetime) every
# cached table a captured launch reads is appended here: the graph bakes the table's raw address, so the tensor must outlive
# its cache entry (the cache holds at most four tables per decoder and evicts on the fifth aux tensor).
CAPTURE_KEEPALIVE = None


def _aux_table_cached(m: "PackedMlp", aux):
    """The per-aux-row layer-1 table of (decoder image, aux tensor version), computed once and kept with the packed decoder
    (which is rebuilt whenever the weights change).  An entry remembers the stream that computed it and an event behind that
    launch: a later user on ANOTHER stream waits for the event first (one model driven from several streams -- two batches in
    flight -- must not read a table whose kernel has not run yet)."""
    cache = m.__dict__.setdefault("_aux_tables", {})
    key = (aux.data_ptr(), aux._version, aux.shape[0])
    capturing = torch.cuda.is_current_stream_capturing()
    hit = cache.get(key)
    if hit is None:
        if capturing:
            # a miss inside a capture: the table is computed by a node of the graph itself and lives in the graph's pool
            # (recomputed per replay; not cached -- an eager call must never see pool memory)
            return mlp_aux_table(m, aux)
        if len(cache) >= 4:
            cache.clear()                # evicted tables stay alive wherever a captured graph holds them (CAPTURE_KEEPALIVE)
        table = mlp_aux_table(m, aux)
        ev = torch.cuda.Event()
        ev.record()
        # the aux tensor is held too: its address cannot be recycled for another tensor while the entry lives
        hit = cache[key] = (aux, table, ev, _raw_stream(torch.cuda.current_device()) if _raw_stream else None)
    elif not capturing and (_raw_stream is None or hit[3] != _raw_stream(torch.cuda.current_device())):
        torch.cuda.current_stream().wait_event(hit[2])
    # (capturing: GraphedRenderer drains the device after its eager warm-up passes and before the capture starts, so a cached
    #  table is complete; an event recorded outside the capture must not be waited on inside it)
    if capturing and CAPTURE_KEEPALIVE is not None:
        CAPTURE_KEEPALIVE.append(hit)
    return hit[1]


def mlp_rows_table(m: "PackedMlp", feat, table, n_dev=None, save_hidden=False):
    """The split-bf16 decoder with ONE table row per decoder row (tir_mlp_[train_]fwd_auxtab_bf16x3, aux_map = NULL): `table`
    [n, 128] carries everything of layer 1 that is not a function of the features -- bias, the aux columns and, for the
    residue-prediction normal decoder, the derived-normal columns.  -> out, or (out, h1, h2) with save_hidden."""
    if MLP_IMPL != "bf16x3":
        raise NotImplementedError("per-row layer-1 tables exist for the split-bf16 decoder only (TENSOIR_MLP=bf16x3)")
    feat = f32(feat, "feat")
    n = feat.shape[0]
    table = f32(table, "table", 128)
    if table.shape[0] != n:
        raise ValueError("table must have one row per feature row")
    out = torch.empty((n, m.out_dim), dtype=torch.float32, device=feat.device)
    if not save_hidden:
        _call("tir_mlp_fwd_auxtab_bf16x3", C.byref(m.desc), _ptr(feat), feat.shape[1], _ptr(table), None, 0, _ptr(out), n,
              _ptr(n_dev), _stream())
        return out
    h1 = torch.empty((n, 128), dtype=torch.float32, device=feat.device)
    h2 = torch.empty((n, 128), dtype=torch.float32, device=feat.device)
    _call("tir_mlp_train_fwd_auxtab_bf16x3", C.byref(m.desc), _ptr(feat), feat.shape[1], _ptr(table), None, 0, _ptr(out),
          _ptr(h1), _ptr(h2), n, _ptr(n_dev), _stream())
    return out, h1, h2


def _stats_ptr(name, dev):
    if STATS is None:
        return None
    if name not in STATS:
        STATS[name] = torch.zeros((1,), dtype=torch.int64, device=dev)
    return C.c_void_p(STATS[name].data_ptr())


def _call(name, *args):
    with _timed(name):
        rc = getattr(lib(), name)(*args)
    check(rc, name)


class _timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if TIMING is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if TIMING is not None:
            self.e1.record()
            TIMING.append((self.name, self.e0, self.e1))
        return False


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t=None):
    """The current HIP stream of the current device as the void* the C ABI takes.  The raw accessor skips the Stream object
    torch.cuda.current_stream() builds per call (~20 calls per step: 10 us -> 1 us each on the host-bound eager path)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class AsyncFloats:
    """A few device floats on their way to the host (capacity.AsyncCount for float tables): copy into pinned memory + event queued NOW.
    Pinned buffers and events are recycled (a training step creates one of these per parameter version)."""
    _free = []

    def __init__(self, t):
        n = t.numel()
        slot = next((k for k, (p, _) in enumerate(AsyncFloats._free) if p.numel() == n), None)
        self.pin, self.ev = AsyncFloats._free.pop(slot) if slot is not None else (torch.empty(n, dtype=torch.float32, pin_memory=True), torch.cuda.Event())
        self.pin.copy_(t.view(-1), non_blocking=True)
        self.ev.record(torch.cuda.current_stream(t.device))
        self.value = None

    def ready(self):
        return self.value is not None or self.ev.query()

    def get(self):
        if self.value is None:
            self.ev.synchronize()
            self.value = self.pin.tolist()
            if len(AsyncFloats._free) < 8:
                AsyncFloats._free.append((self.pin, self.ev))
            self.pin = self.ev = None
        return self.value


class HalfRange:
    """Range guard of one fp16 shadow of the field (tir_pack_half_checked's RANGE CONTRACT): the abs-maxima of the three
    appearance planes, the three lines, the light rows and basis_mat^T travel to the host behind the pack launch; ok() is
    True when no plane * line product, no plane * line * light-row product and no basis_mat element can leave the finite fp16
    range: bound = max_i (max|plane_i| max|line_i|) max(1, max|light row|) < INDIRECT_PROBE["range"]."""

    def __init__(self, absmax):
        self.pending = AsyncFloats(absmax)
        self.maxima = self.bound = self.result = None

    def ready(self):
        return self.result is not None or self.pending.ready()

    @staticmethod
    def judge(m, lim):
        """m = [max|plane_0..2|, max|line_0..2|, max|light rows|, max|basis_mat|] -> (ok, bound).  The packed-fp16 gather forms
        (plane x line) in fp16 BEFORE the light row is applied (h16_chunk_pk), so the bound carries max(1, light).  A NaN maximum
        fails every comparison."""
        bound = max(m[i] * m[3 + i] for i in range(3)) * max(1.0, m[6])
        return bool(bound < lim and m[7] < lim and all(v < lim for v in m[:7])), bound

    def ok(self):
        if self.result is None:
            m = self.pending.get()
            self.maxima = {"plane": m[0:3], "line": m[3:6], "light": m[6], "basis": m[7]}
            self.result, self.bound = HalfRange.judge(m, INDIRECT_PROBE["range"])
        return self.result


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _req(t, dtype, name, last=None):
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise _lib.TensoirHipError(f"{name}: tensor must live on the GPU (got {t.device}); "
                                   "tensoir_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if last is not None and (t.dim() < 1 or t.shape[-1] != last):
        raise ValueError(f"{name}: last dim must be {last}, got {tuple(t.shape)}")
    return t if t.is_contiguous() else t.contiguous()


def f32(t, name, last=None):
    return _req(t, torch.float32, name, last)


def i32(t, name):
    return _req(t, torch.int32, name)


def to_device(t, device, dtype=None):
    """`t.to(device, dtype)` that does not stall the launch queue: a host tensor goes through pinned memory and a
    non-blocking copy (a pageable-memory copy waits for everything queued on the stream before it returns)."""
    device = torch.device(device)
    if t.device.type == "cpu" and device.type == "cuda":
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        return t.contiguous().pin_memory().to(device, non_blocking=True)
    return t.to(device) if dtype is None else t.to(device, dtype)


def record_check(counters, caps, state, host_out):
    """One kernel: device record counters -> pinned host_out (counts [0:4], running maxima [4:8], sticky overflow flag
    [8]); `state` = device int64[5] holding the maxima and the flag across launches."""
    n = len(counters)
    for t in counters:
        if t.dtype != torch.int32 or not t.is_cuda:
            raise _lib.TensoirHipError("record_check: counters must be int32 device tensors")
    if not host_out.is_pinned() or host_out.dtype != torch.int64 or host_out.numel() < 9:
        raise _lib.TensoirHipError("record_check: host_out must be a pinned int64[9] tensor")
    if state.dtype != torch.int64 or state.numel() < 5 or not state.is_cuda:
        raise _lib.TensoirHipError("record_check: state must be a device int64[5] tensor")
    ptrs = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in counters])
    cap_arr = (C.c_int64 * max(n, 1))(*[int(c) for c in caps])
    _call("tir_record_check", ptrs, cap_arr, n, _ptr(state), C.c_void_p(host_out.data_ptr()), _stream())


# ---- packing ------------------------------------------------------------------------------------
def pack_plane(src):
    """[1,C,H,W] (or [C,H,W]) -> channel-last [H,W,C]."""
    src = f32(src.detach(), "plane")
    c, h, w = src.shape[-3:]
    dst = torch.empty((h, w, c), dtype=torch.float32, device=src.device)
    _call("tir_pack_plane", _ptr(src), _ptr(dst), c, h, w, _stream())
    return dst


def pack_half(tables, scan=()):
    """fp16 copies (round to nearest even, SATURATING, same element order) of up to 8 fp32 tensors in ONE launch
    (tir_pack_half_checked) -> (copies, absmax): absmax[i] = max |x| of tables[i], then of every tensor in `scan` (tables whose
    range matters but which the kernels read as fp32: light rows, basis_mat) -- a device tensor, read by the range guard of the
    indirect-light precision policy (relight.HalfRange); a NaN anywhere in a table shows as NaN."""
    tables = [t.detach() for t in tables]
    scan = [t.detach() for t in scan]
    for t in tables + scan:
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError("pack_half: fp32 CUDA tensors expected")
    # same strides as the source (the channel-last planes keep their layout): a raw element-for-element copy of the storage
    outs = [torch.empty_strided(t.shape, t.stride(), dtype=torch.float16, device=t.device) for t in tables]
    k = len(tables) + len(scan)
    srcs = (C.c_void_p * k)(*[t.data_ptr() for t in tables + scan])
    dsts = (C.c_void_p * k)(*([o.data_ptr() for o in outs] + [None] * len(scan)))
    cnts = (C.c_int64 * k)(*[_storage_span(t) for t in tables + scan])
    absmax = torch.zeros((k,), dtype=torch.float32, device=(tables + scan)[0].device)
    _call("tir_pack_half_checked", srcs, dsts, cnts, k, _ptr(absmax), _stream())
    return outs, absmax


def _storage_span(t):
    """Elements between the first and the last element of a dense (possibly permuted) tensor."""
    n = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
    if n != t.numel():
        raise ValueError("pack_half: dense tensors expected")
    return n


def pack_occupancy(vol):
    """[.., D, H, W] float 0/1 volume -> (D+1)(H+1)(W+1) neighbourhood bytes."""
    vol = f32(vol.detach(), "alpha_volume")
    D, H, W = vol.shape[-3:]
    nbr = torch.empty(((D + 1) * (H + 1) * (W + 1),), dtype=torch.uint8, device=vol.device)
    _call("tir_pack_occupancy", _ptr(vol), _ptr(nbr), W, H, D, _stream())
    return nbr


def pack_basis(w):
    w = f32(w.detach(), "basis_mat.weight")
    app_dim, n_in = w.shape
    dst = torch.empty((n_in, 32), dtype=torch.float32, device=w.device)
    _call("tir_pack_basis", _ptr(w), _ptr(dst), app_dim, n_in, _stream())
    return dst


def light_mean(ll):
    ll = f32(ll.detach(), "light_line.weight")
    L, n = ll.shape
    out = torch.empty((n,), dtype=torch.float32, device=ll.device)
    _call("tir_light_mean", _ptr(ll), _ptr(out), L, n, _stream())
    return out


def pack_mlp(w0, b0, w1, b1, w2, b2, feat_dim, pe):
    ws = [f32(t.detach(), "mlp weight") for t in (w0, b0, w1, b1, w2, b2)]
    hidden, out_dim = w1.shape[0], w2.shape[0]
    n = lib().tir_mlp_packed_floats(feat_dim, pe, hidden, out_dim)
    if n < 0:
        check(int(n), f"tir_mlp_packed_floats(feat={feat_dim}, pe={pe}, hidden={hidden}, out={out_dim})")
    if tuple(w0.shape) != (hidden, feat_dim + 3 + 2 * pe * feat_dim + 2 * pe * 3):
        raise ValueError(f"mlp.0.weight has shape {tuple(w0.shape)}")
    packed = torch.empty((int(n),), dtype=torch.float32, device=w0.device)
    _call("tir_pack_mlp", *[_ptr(t) for t in ws], feat_dim, pe, hidden, out_dim, _ptr(packed),
                             _stream())
    return packed


class PackedMlp:
    def __init__(self, seq, feat_dim, pe, act, w0=None):
        """seq: the reference's nn.Sequential(Linear, ReLU, Linear, ReLU, Linear); w0: layer-1 weights in the kernels' column
        order [feat, aux, PE(feat), PE(aux)] when the module stores them differently (the residue-prediction normal decoder)."""
        self.packed = pack_mlp(seq[0].weight if w0 is None else w0, seq[0].bias, seq[2].weight, seq[2].bias,
                               seq[4].weight, seq[4].bias, feat_dim, pe)
        self.out_dim = seq[4].weight.shape[0]
        self.desc = TirMlp(self.packed.data_ptr(), feat_dim, pe, seq[2].weight.shape[0],
                           self.out_dim, act, TUNE["mlp_grid"])


# ---- field kernels --------------------------------------------------------------------------------
def vm_density(field: TirField, xyz, want_feat=True, want_sigma=False):
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    feat = torch.empty((n,), dtype=torch.float32, device=xyz.device) if want_feat else None
    sigma = torch.empty((n,), dtype=torch.float32, device=xyz.device) if want_sigma else None
    _call("tir_vm_density_fwd", C.byref(field), _ptr(xyz), _ptr(feat), _ptr(sigma), n, _stream())
    return feat, sigma


def dense_sigma_build(field: TirField, device):
    """The dense density-feature volume of `field` (tir_dense_sigma_build): fp32 [grid z][grid y][grid x + 1] and its row pitch."""
    X, Y, Z = [int(g) for g in field.grid]
    pitch = X + 1
    vol = torch.empty((Z, Y, pitch), dtype=torch.float32, device=device)
    _call("tir_dense_sigma_build", C.byref(field), _ptr(vol), pitch, _stream())
    return vol, pitch


def dense_app_bytes(field: TirField):
    """Size of the dense appearance-feature volume of `field`: 64 bytes per corner, rows of grid x + 1 corners."""
    X, Y, Z = [int(g) for g in field.grid]
    return 64 * (X + 1) * Y * Z


def dense_app_build(field: TirField, device):
    """The dense appearance-feature volume of a one-light `field` (tir_dense_app_build): fp16 [grid z][grid y][grid x + 1][2][16]
    and its row pitch in corners."""
    X, Y, Z = [int(g) for g in field.grid]
    pitch = X + 1
    vol = torch.empty((Z, Y, pitch, 2, 16), dtype=torch.float16, device=device)
    _call("tir_dense_app_build", C.byref(field), _ptr(vol), pitch, _stream())
    return vol, pitch


def dense_sigma(field: TirField, xyz, want_feat=True, want_sigma=False):
    """vm_density through the trilinear lookup of field.dense_sigma (the dense secondary march's arithmetic)."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    feat = torch.empty((n,), dtype=torch.float32, device=xyz.device) if want_feat else None
    sigma = torch.empty((n,), dtype=torch.float32, device=xyz.device) if want_sigma else None
    _call("tir_dense_sigma_fwd", C.byref(field), _ptr(xyz), _ptr(feat), _ptr(sigma), n, _stream())
    return feat, sigma


def occupancy_query(field: TirField, xyz):
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    hit = torch.empty((n,), dtype=torch.uint8, device=xyz.device)
    _call("tir_occupancy_query", C.byref(field), _ptr(xyz), _ptr(hit), n, _stream())
    return hit


def dense_alpha(field: TirField, grid_size, length):
    """getDenseAlpha: alpha [gx,gy,gz] on the lattice aabb0*(1-s)+aabb1*s, s = torch.linspace(0,1,g) per axis."""
    gx, gy, gz = [int(g) for g in grid_size]
    dev = torch.device("cuda", torch.cuda.current_device())
    lins = [torch.linspace(0, 1, g).to(dev).contiguous() for g in (gx, gy, gz)]
    alpha = torch.empty((gx, gy, gz), dtype=torch.float32, device=dev)
    _call("tir_dense_alpha", C.byref(field), _ptr(lins[0]), _ptr(lins[1]), _ptr(lins[2]), gx, gy, gz, float(length),
          _ptr(alpha), _stream())
    return alpha, lins


def alpha_pool(alpha, thres):
    """updateAlphaMask's pool + threshold: alpha [gx,gy,gz] -> (volume [gz,gy,gx] float 0/1, index bbox int32[6])."""
    alpha = f32(alpha, "alpha")
    gx, gy, gz = alpha.shape
    vol = torch.empty((gz, gy, gx), dtype=torch.float32, device=alpha.device)
    bbox = torch.tensor([2 ** 31 - 1] * 3 + [-1] * 3, dtype=torch.int32, device=alpha.device)
    _call("tir_alpha_pool", _ptr(alpha), gx, gy, gz, float(thres), _ptr(vol), _ptr(bbox), _stream())
    return vol, bbox


def filter_rays(field: TirField, rays, n_samples, bbox_only):
    rays = f32(rays, "rays", 6)
    n = rays.shape[0]
    mask = torch.empty((n,), dtype=torch.uint8, device=rays.device)
    _call("tir_filter_rays", C.byref(field), _ptr(rays), n, int(n_samples), int(bool(bbox_only)), _ptr(mask), _stream())
    return mask.bool()


def density_grad(field: TirField, xyz, want_sigma=False, want_grad=False, want_normal=True, n_dev=None):
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    mk = lambda on, *s: torch.empty(s, dtype=torch.float32, device=xyz.device) if on else None
    sigma, grad, normal = mk(want_sigma, n), mk(want_grad, n, 3), mk(want_normal, n, 3)
    _call("tir_density_grad_fwd", C.byref(field), _ptr(xyz), _ptr(sigma), _ptr(grad), _ptr(normal),
                                     n, _ptr(n_dev), _stream())
    return sigma, grad, normal


FEAT_STRIDE = 32     # feature rows are padded to 128 bytes (aligned float4 stores / loads)
# "mfma" (exact fp32 matrix-core contraction), "bf16x3" (split-bf16 matrix cores, parity grade) or "valu" (cross-check)
APP_ENTRY = {"mfma": "tir_vm_app_fwd", "x3": "tir_vm_app_fwd_x3", "bf16x3": "tir_vm_app_fwd_bf16x3", "valu": "tir_vm_app_fwd_valu"}
APP_IMPL = os.environ.get("TENSOIR_APP", "mfma")


def vm_app(field: TirField, xyz, light_idx=None, idx_map=None, want_rad=True, want_int=False, impl=None,
           idx_div=0, n_dev=None):
    """Returns padded feature buffers [n, FEAT_STRIDE]; columns >= app_dim are zero.
    n_dev (int32 device scalar): only the first min(n, n_dev) rows are computed (rest left uninitialised)."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    ad = FEAT_STRIDE
    if want_rad:
        if light_idx is None:
            raise ValueError("light_idx is required for the radiance feature")
        light_idx = i32(light_idx, "light_idx").view(-1)
        if idx_map is not None:
            idx_map = i32(idx_map, "idx_map").view(-1)
            if idx_map.numel() != n:
                raise ValueError("idx_map must have one entry per point")
        elif light_idx.numel() != n and idx_div <= 1:
            raise ValueError("light_idx must have one entry per point")
    rad = torch.empty((n, ad), dtype=torch.float32, device=xyz.device) if want_rad else None
    intr = torch.empty((n, ad), dtype=torch.float32, device=xyz.device) if want_int else None
    if impl is None:       # the default route follows the contraction setting (x3 unless the exact decoders / fp32 contraction are selected)
        impl = "x3" if (APP_IMPL == "mfma" and app_contraction() == "x3" and int(field.n_acomp) in (16, 24, 48)) else APP_IMPL
    _call(APP_ENTRY[impl], C.byref(field), _ptr(xyz),
          _ptr(light_idx) if want_rad else None, _ptr(idx_map) if want_rad else None, _ptr(rad), _ptr(intr),
          ad, int(idx_div), n, _ptr(n_dev), _stream())
    return rad, intr


def vm_app_h16(field: TirField, fh: TirFieldHalf, xyz, light_idx, idx_map=None, idx_div=0, n_dev=None):
    """Radiance features [n, FEAT_STRIDE] from the fp16 shadow of the appearance planes / lines (tir_vm_app_fwd_h16): the
    indirect-light precision policy's gather (48 appearance components per plane only)."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    light_idx = i32(light_idx, "light_idx").view(-1)
    if idx_map is not None:
        idx_map = i32(idx_map, "idx_map").view(-1)
        if idx_map.numel() != n:
            raise ValueError("idx_map must have one entry per point")
    elif light_idx.numel() != n and idx_div <= 1:
        raise ValueError("light_idx must have one entry per point")
    rad = torch.empty((n, FEAT_STRIDE), dtype=torch.float32, device=xyz.device)
    _call("tir_vm_app_fwd_h16", C.byref(field), C.byref(fh), _ptr(xyz), _ptr(light_idx), _ptr(idx_map), _ptr(rad), FEAT_STRIDE,
          int(idx_div), n, _ptr(n_dev), _stream())
    return rad


def indirect_fused(field: TirField, fh: TirFieldHalf, m: "PackedMlp", xyz, light_idx, rec_map, idx_div, dirs, n_dirs, n_dev=None):
    """Radiance [n, out_dim] of the secondary-ray records in ONE launch (tir_indirect_fused_fwd): fp16-shadow appearance gather,
    basis_mat contraction and the radiance decoder, the feature rows staying in registers.  rec_map[s] = pair id of record s:
    light index = light_idx[pair // idx_div], view direction = dirs[pair % n_dirs] (through the cached aux table)."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    light_idx = i32(light_idx, "light_idx").view(-1)
    rec_map = i32(rec_map, "rec_map").view(-1)
    if rec_map.numel() != n:
        raise ValueError("rec_map must have one entry per record")
    dirs = f32(dirs, "dirs", 3)
    table = _aux_table_cached(m, dirs)
    out = torch.empty((n, m.out_dim), dtype=torch.float32, device=xyz.device)
    _call("tir_indirect_fused_fwd", C.byref(field), C.byref(fh), C.byref(m.desc), _ptr(xyz), _ptr(light_idx), _ptr(rec_map), int(idx_div),
          int(n_dirs), _ptr(table), _ptr(out), n, _ptr(n_dev), _stream())
    return out


def indirect_fused_hp(field: TirField, m: "PackedMlp", xyz, light_idx, rec_map, idx_div, dirs, n_dirs, n_dev=None):
    """indirect_fused at the precision a trained checkpoint needs (tir_indirect_fused_hp_fwd): fp32 taps, fp16 hi + lo contraction,
    decoder weights as fp16 + fp8 residue -- the auto policy's first fallback, one launch instead of gather + decoder with the
    feature rows through HBM."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    light_idx = i32(light_idx, "light_idx").view(-1)
    rec_map = i32(rec_map, "rec_map").view(-1)
    if rec_map.numel() != n:
        raise ValueError("rec_map must have one entry per record")
    dirs = f32(dirs, "dirs", 3)
    table = _aux_table_cached(m, dirs)
    out = torch.empty((n, m.out_dim), dtype=torch.float32, device=xyz.device)
    _call("tir_indirect_fused_hp_fwd", C.byref(field), C.byref(m.desc), _ptr(xyz), _ptr(light_idx), _ptr(rec_map), int(idx_div),
          int(n_dirs), _ptr(table), _ptr(out), n, _ptr(n_dev), _stream())
    return out


# decoder implementations: "mfma" = exact fp32 matrix cores, "bf16x3" = split-bf16 matrix cores (parity
# grade, ~5x fewer MFMA cycles), "bf16" = single-product reduced precision, "valu" = cross-check kernel
MLP_ENTRY = {"mfma": "tir_mlp_fwd", "bf16x3": "tir_mlp_fwd_bf16x3", "bf16": "tir_mlp_fwd_bf16",
             "valu": "tir_mlp_fwd_valu"}
MLP_IMPL = os.environ.get("TENSOIR_DECODER", "bf16x3")
if MLP_IMPL not in MLP_ENTRY:
    raise ValueError(f"TENSOIR_DECODER={MLP_IMPL!r}: expected one of {sorted(MLP_ENTRY)}")
# Knobs of the precision policy for INDIRECT light; the policy itself and its description: tensoir_amd/indirect.py.
_IND = os.environ.get("TENSOIR_INDIRECT_PRECISION", "auto")
if _IND not in ("auto", "f16", "hp", "full"):
    raise ValueError(f"TENSOIR_INDIRECT_PRECISION={_IND!r}: expected auto, f16, hp or full")
SECONDARY_MLP_IMPL = {"full": None, "hp": "hp"}.get(_IND, "f16")       # None | "f16" | "hp" | "bf16" (probe only) | "bf16x3"; read by indirect.mode
SECONDARY_APP_IMPL = "h16" if _IND in ("auto", "f16") else None        # None | "h16"; read by indirect.mode
INDIRECT_GUARD = _IND == "auto"        # False: the settings above apply unconditionally (f16 / hp: the caller vouches for range and precision); indirect.mode
INDIRECT_HP = os.environ.get("TENSOIR_INDIRECT_HP", "1") != "0"        # the hp tier of the auto policy (indirect.establish's try_hp)
# limits of the self-check and of the range guard (tensoir_amd/indirect.py: establish, record_estimate; HalfRange above)
INDIRECT_PROBE = {"map_limit": float(os.environ.get("TENSOIR_INDIRECT_MAP_LIMIT", "2.5e-5")), "train_map_limit": 1.0e-4, "records": 32768, "interval": 64, "w_bias": 0.5, "w_rms": 0.25, "w_max": 0.25, "limit": 2.5e-5,
                  "range": 6.0e4}


# TENSOIR_FUSED_INDIRECT=0: gather and decoder of the secondary-ray records as two launches (tir_vm_app_fwd_h16 +
# tir_mlp_fwd_auxtab_f16, features through HBM) instead of the fused kernel (tir_indirect_fused_fwd).  Only meaningful under the f16 policy.
FUSED_INDIRECT = os.environ.get("TENSOIR_FUSED_INDIRECT", "1") != "0"


def fused_indirect():
    return FUSED_INDIRECT and AUX_TABLE and secondary_app_impl() == "h16" and secondary_mlp_impl() == "f16"


def full_indirect_route():
    """Which launches decode the secondary-ray records when the indirect-light policy says `full` (reported by bench.py)."""
    gather = "tir_vm_app_fwd_x3 (fp32 taps, fp16 hi + lo contraction)" if app_contraction() == "x3" else "tir_vm_app_fwd (fp32 taps, fp32 MFMA contraction)"
    return gather + " + tir_mlp_fwd_auxtab_bf16x3 (split-bf16 x3), feature rows through HBM"


def hp_indirect_route():
    return ("tir_indirect_fused_hp_fwd: fp32 taps, fp16 hi + lo basis contraction, decoder with fp16 activations and fp16 + fp8-residue "
            "weights (residue on the block-scaled fp8 matrix instruction), one launch, feature rows in registers")


def secondary_app_impl():
    """Gather mode of the secondary-record radiance features under the current settings."""
    return SECONDARY_APP_IMPL if (MLP_IMPL == "bf16x3" and SECONDARY_APP_IMPL) else None


def secondary_mlp_impl():
    """Decoder mode of the secondary-record radiance launch under the current settings."""
    return SECONDARY_MLP_IMPL if (MLP_IMPL == "bf16x3" and SECONDARY_MLP_IMPL) else None


def mlp_multi(jobs, n_dev=None, save_hidden=False):
    """Several decoders over the same rows in one launch (tir_mlp_fwd_multi_bf16x3).  jobs: list of up to four
    (PackedMlp, feat [n, FEAT_STRIDE], aux [*, 3], aux_map or None); returns the list of outputs [n, out_dim] -- with
    save_hidden (training forward, tir_mlp_train_fwd_multi_bf16x3) the list of (out, h1 [n,128], h2 [n,128])."""
    n = jobs[0][1].shape[0]
    k = len(jobs)
    feats, auxs, maps, outs = [], [], [], []
    for m, feat, aux, aux_map in jobs:
        feat = f32(feat, "feat")
        if feat.shape[0] != n or feat.dim() != 2 or feat.shape[1] != FEAT_STRIDE:
            raise ValueError(f"mlp_multi: every job needs [n, {FEAT_STRIDE}] feature rows")
        aux = f32(aux, "aux", 3)
        if aux_map is not None:
            aux_map = i32(aux_map, "aux_map").view(-1)
        elif aux.shape[0] != n:
            raise ValueError("aux must have one row per feature row (or pass aux_map)")
        feats.append(feat); auxs.append(aux); maps.append(aux_map)
        outs.append(torch.empty((n, m.out_dim), dtype=torch.float32, device=feat.device))
    arr = lambda ts: (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts])
    descs = (C.POINTER(TirMlp) * k)(*[C.pointer(m.desc) for m, _, _, _ in jobs])
    # Off by default in the merged primary-stage launch: one job in four would save 12 of its 216 MFMAs per tile (~2 us at
    # 230 k rows) while its per-ray table costs a 9 us launch of its own.  AUX_TABLE_MULTI = True selects it (tests do).
    use_tab = [AUX_TABLE and AUX_TABLE_MULTI and not save_hidden and mp is not None and aux.shape[0] * 8 <= max(n, 1)
               for aux, mp in zip(auxs, maps)]
    if any(use_tab):
        # jobs whose aux rows come through an index map with few distinct rows (same rule as mlp()): aux-table variant of layer 1
        tables = [mlp_aux_table(m, aux) if t else None for (m, _, _, _), aux, t in zip(jobs, auxs, use_tab)]
        _call("tir_mlp_fwd_multi_auxtab_bf16x3", descs, arr(feats), FEAT_STRIDE, arr(auxs), arr(maps), arr(tables), arr(outs), k, n,
              _ptr(n_dev), _stream())
        return outs
    if save_hidden:
        h1s = [torch.empty((n, 128), dtype=torch.float32, device=outs[0].device) for _ in range(k)]
        h2s = [torch.empty((n, 128), dtype=torch.float32, device=outs[0].device) for _ in range(k)]
        _call("tir_mlp_train_fwd_multi_bf16x3", descs, arr(feats), FEAT_STRIDE, arr(auxs), arr(maps), arr(outs), arr(h1s), arr(h2s),
              k, n, _ptr(n_dev), _stream())
        return list(zip(outs, h1s, h2s))
    _call("tir_mlp_fwd_multi_bf16x3", descs, arr(feats), FEAT_STRIDE, arr(auxs), arr(maps), arr(outs), k, n, _ptr(n_dev),
          _stream())
    return outs


def mlp(m: PackedMlp, feat, aux, aux_map=None, impl=None, aux_mod=0, n_dev=None):
    impl = impl or MLP_IMPL
    feat = f32(feat, "feat")
    if feat.dim() != 2 or feat.shape[1] < m.desc.feat_dim:
        raise ValueError(f"feat: expected [n, >= {m.desc.feat_dim}], got {tuple(feat.shape)}")
    aux = f32(aux, "aux", 3)
    n = feat.shape[0]
    if aux_map is not None:
        aux_map = i32(aux_map, "aux_map").view(-1)
        if aux_map.numel() != n:
            raise ValueError("aux_map must have one entry per row")
    elif aux.shape[0] != n and aux_mod <= 0:
        raise ValueError("aux must have one row per feature row")
    out = torch.empty((n, m.out_dim), dtype=torch.float32, device=feat.device)
    f16 = impl == "f16"
    if f16:
        impl = "bf16x3"              # rows that do not qualify for the aux-table launch below take the parity-grade kernel
    if impl == "bf16x3" and AUX_TABLE and (aux_map is not None or aux_mod > 0) and aux.shape[0] * 8 <= max(n, 1):
        # few distinct aux rows (one per ray / light direction) for many decoder rows: their 15 input columns + the bias as a
        # per-aux-row start value of the layer-1 accumulators, 9 instead of 10 k-blocks of matrix work per row
        # the light-direction grid of a scene is a persistent tensor: its table is computed once per (decoder image, aux tensor
        # version) and kept with the packed decoder (which is rebuilt whenever the weights change)
        table = _aux_table_cached(m, aux)
        _call("tir_mlp_fwd_auxtab_f16" if f16 else "tir_mlp_fwd_auxtab_bf16x3", C.byref(m.desc), _ptr(feat), feat.shape[1], _ptr(table),
              _ptr(aux_map), int(aux_mod), _ptr(out), n, _ptr(n_dev), _stream())
        return out
    _call(MLP_ENTRY[impl], C.byref(m.desc), _ptr(feat), feat.shape[1], _ptr(aux),
          _ptr(aux_map), int(aux_mod), _ptr(out), n, _ptr(n_dev), _stream())
    return out


# ---- primary march --------------------------------------------------------------------------------
def march_primary(field: TirField, rays, ray_jitter, n_samples, t_stop):
    rays = f32(rays, "rays", 6)
    B = rays.shape[0]
    dev = rays.device
    if ray_jitter is not None:
        ray_jitter = f32(ray_jitter, "ray_jitter").view(-1)
        if ray_jitter.numel() != B:
            raise ValueError("ray_jitter must be [B] / [B,1]")
    weight = torch.empty((B, n_samples), dtype=torch.float32, device=dev)
    acc = torch.empty((B,), dtype=torch.float32, device=dev)
    depth = torch.empty((B,), dtype=torch.float32, device=dev)
    tend = torch.empty((B,), dtype=torch.float32, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("tir_march_primary_fwd", C.byref(field), _ptr(rays), _ptr(ray_jitter), B, n_samples,
                                      float(t_stop), _ptr(weight), _ptr(acc), _ptr(depth), _ptr(tend),
                                      _ptr(cnt), _stats_ptr("tir_march_primary_fwd", dev), _stream())
    return weight, acc, depth, tend, cnt


def march_primary_fused(field: TirField, rays, n_samples, t_stop, cap, words):
    """Inference-only primary march that also emits the view-direction table, re-arms the pass counters and scans the
    record counts (tir_march_primary_fused_fwd).  words: persistent int32[8] of the model -- [1:3] secondary record
    counter (zeroed here), [3] scan ticket, [5] record total.  Returns weight, acc, depth, cnt, offsets, total, viewdirs."""
    rays = f32(rays, "rays", 6)
    B = rays.shape[0]
    dev = rays.device
    weight = torch.empty((B, n_samples), dtype=torch.float32, device=dev)
    acc = torch.empty((B,), dtype=torch.float32, device=dev)
    depth = torch.empty((B,), dtype=torch.float32, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    off = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    vd = torch.empty((B, 3), dtype=torch.float32, device=dev)
    total = words[5:6]
    _call("tir_march_primary_fused_fwd", C.byref(field), _ptr(rays), None, B, n_samples, float(t_stop), _ptr(weight),
          _ptr(acc), _ptr(depth), None, _ptr(cnt), _stats_ptr("tir_march_primary_fwd", dev), _ptr(vd),
          C.c_void_p(words.data_ptr() + 4), 2, C.c_void_p(words.data_ptr() + 12), _ptr(off), int(cap), _ptr(total), _stream())
    return weight, acc, depth, cnt, off, total, vd


def composite_primary_fused(rays, offsets, rec_w, rgb, brdf, brdf_jit, pred_n, der_n, acc, depth, white_bg, is_relight,
                            fixed_fresnel, words, rng_state=None, rng_step=0):
    """tir_composite_primary_fused: map rows + the two smoothness means (float32[2]); words[4] is the ticket."""
    rays = f32(rays, "rays", 6)
    B = rays.shape[0]
    out = torch.empty((B, MAP_STRIDE), dtype=torch.float32, device=rays.device)
    smooth = torch.zeros((2,), dtype=torch.float32, device=rays.device) if B == 0 else \
        torch.empty((2,), dtype=torch.float32, device=rays.device)
    _call("tir_composite_primary_fused", _ptr(rays), _ptr(offsets), _ptr(rec_w), _ptr(rgb), _ptr(brdf), _ptr(brdf_jit),
          _ptr(pred_n), _ptr(der_n), _ptr(acc), _ptr(depth), B, int(bool(white_bg)), int(bool(is_relight)),
          float(fixed_fresnel), _ptr(out), C.c_void_p(words.data_ptr() + 16), _ptr(smooth), _ptr(rng_state), int(rng_step),
          _stream())
    return out, smooth


def vm_app_jitter(field: TirField, xyz, scale, seed, offset, rng_state=None, n_dev=None):
    """Intrinsic features of xyz + scale * N(0,1), noise drawn in the kernel (tir_vm_app_jitter_fwd).
    Returns (xyz_jittered [n,3], int_feat [n, FEAT_STRIDE])."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    xyz_j = torch.empty_like(xyz)
    intr = torch.empty((n, FEAT_STRIDE), dtype=torch.float32, device=xyz.device)
    _call("tir_vm_app_jitter_fwd", C.byref(field), _ptr(xyz), n, _ptr(n_dev), float(scale), int(seed) & (2 ** 64 - 1),
          int(offset) & (2 ** 64 - 1), _ptr(rng_state), _ptr(xyz_j), _ptr(intr), FEAT_STRIDE, _stream())
    return xyz_j, intr


# Contraction of the primary stage's merged gather: "fp32" = the exact-fp32 matrix instruction (tir_vm_app_primary_fwd, the default),
# "x3" = fp16 hi + lo operands, three matrix products (tir_vm_app_primary_x3_fwd / tir_vm_app_fwd_x3).  Round 6 built x3 expecting
# the exact instruction (vector rate) to bind the launch; measured, the launch went from 99 to 96 us only, and on a checkpoint
# trained to 300^3 the albedo / roughness maps moved to 1.0e-4 / 8.5e-5 from the oracle (2e-6 with fp32): the fp16 RESIDUE of a
# product below 0.125 is a subnormal, so the features are good to ~1e-6 of their scale, not 2^-21, and the BRDF decoder of a trained
# field amplifies that ~100-fold (profiles/r06m_precision_trained_300_x3_gather.json).  Opt-in only.
APP_CONTRACTION = os.environ.get("TENSOIR_APP_CONTRACTION", "fp32")
if APP_CONTRACTION not in ("x3", "fp32"):
    raise ValueError(f"TENSOIR_APP_CONTRACTION={APP_CONTRACTION!r}: expected x3 or fp32")


def app_contraction():
    return APP_CONTRACTION if MLP_IMPL == "bf16x3" else "fp32"


def vm_app_primary(field: TirField, xyz, light_idx, idx_map, scale, rng_state, n_dev=None, exact=False):
    """The primary stage's two appearance gathers in one launch (tir_vm_app_primary_x3_fwd / tir_vm_app_primary_fwd): returns
    (rad [n, FEAT_STRIDE], intr, xyz_jittered [n, 3], intr_jittered).  exact: the fp32 contraction whatever the setting (the
    training forward: its saved features feed the hand-written backward)."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    dev = xyz.device
    rad = torch.empty((n, FEAT_STRIDE), dtype=torch.float32, device=dev)
    intr = torch.empty((n, FEAT_STRIDE), dtype=torch.float32, device=dev)
    intr_j = torch.empty((n, FEAT_STRIDE), dtype=torch.float32, device=dev)
    xyz_j = torch.empty_like(xyz)
    _call("tir_vm_app_primary_fwd" if (exact or app_contraction() == "fp32") else "tir_vm_app_primary_x3_fwd", C.byref(field), _ptr(xyz),
          _ptr(i32(light_idx, "light_idx").view(-1)),
          _ptr(None if idx_map is None else i32(idx_map, "idx_map").view(-1)), _ptr(rad), _ptr(intr), FEAT_STRIDE, n, _ptr(n_dev),
          float(scale), 0, 0, _ptr(rng_state), _ptr(xyz_j), _ptr(intr_j), _stream())
    return rad, intr, xyz_j, intr_j


def exclusive_scan(counts):
    counts = i32(counts, "counts").view(-1)
    n = counts.numel()
    off = torch.empty((n + 1,), dtype=torch.int32, device=counts.device)
    _call("tir_exclusive_scan", _ptr(counts), _ptr(off), n, _stream())
    return off


def exclusive_scan_capped(counts, cap):
    """offsets clamped to `cap` records + the true total (device int32 [1])."""
    counts = i32(counts, "counts").view(-1)
    n = counts.numel()
    off = torch.empty((n + 1,), dtype=torch.int32, device=counts.device)
    total = torch.empty((1,), dtype=torch.int32, device=counts.device)
    _call("tir_exclusive_scan_capped", _ptr(counts), _ptr(off), n, int(cap), _ptr(total), _stream())
    return off, total


def compact_primary(field: TirField, rays, ray_jitter, weight, offsets, total, out=None):
    """out: caller-owned (rec_ray, rec_k, rec_w, rec_xyz) of at least offsets[-1] records, written in place of fresh buffers."""
    rays = f32(rays, "rays", 6)
    B, S = weight.shape
    dev = rays.device
    if ray_jitter is not None:
        ray_jitter = f32(ray_jitter, "ray_jitter").view(-1)
    if out is not None:
        rec_ray, rec_k, rec_w, rec_xyz = i32(out[0], "rec_ray"), i32(out[1], "rec_k"), f32(out[2], "rec_w"), f32(out[3], "rec_xyz", 3)
        if min(rec_ray.numel(), rec_k.numel(), rec_w.numel(), rec_xyz.shape[0]) < total:
            raise ValueError("compact_primary: out buffers hold fewer than `total` records")
    else:
        rec_ray = torch.empty((total,), dtype=torch.int32, device=dev)
        rec_k = torch.empty((total,), dtype=torch.int32, device=dev)
        rec_w = torch.empty((total,), dtype=torch.float32, device=dev)
        rec_xyz = torch.empty((total, 3), dtype=torch.float32, device=dev)
    if total > 0:
        _call("tir_compact_primary", C.byref(field), _ptr(rays), _ptr(ray_jitter), _ptr(weight),
                                        _ptr(offsets), B, S, _ptr(rec_ray), _ptr(rec_k), _ptr(rec_w),
                                        _ptr(rec_xyz), _stream())
    return rec_ray, rec_k, rec_w, rec_xyz


def composite_primary(rays, offsets, rec_w, rgb, brdf, brdf_jit, pred_n, der_n, acc, depth,
                      white_bg, is_relight, fixed_fresnel):
    rays = f32(rays, "rays", 6)
    B = rays.shape[0]
    out = torch.empty((B, MAP_STRIDE), dtype=torch.float32, device=rays.device)
    _call("tir_composite_primary", _ptr(rays), _ptr(offsets), _ptr(rec_w), _ptr(rgb), _ptr(brdf),
                                      _ptr(brdf_jit), _ptr(pred_n), _ptr(der_n), _ptr(acc), _ptr(depth),
                                      B, int(bool(white_bg)), int(bool(is_relight)),
                                      float(fixed_fresnel), _ptr(out), _stream())
    return out


# ---- secondary march ------------------------------------------------------------------------------
def march_secondary(field: TirField, origins, dirs, z_vals, n_rays, org_map=None, dir_map=None,
                    active=None, t_stop=0.0, want_records=False, rec_cap=0, want_nerfactor=True, n_dirs=0,
                    ray_ids=None, n_ids_dev=None, vis=None, rec_cnt=None, counter=None, oma=None, rec=None):
    """ray_ids / n_ids_dev: march only the listed pair ids (tir_march_secondary_ids_fwd); vis / rec_cnt / oma: pre-filled
    per-pair buffers (shade_setup_compact wrote the masked pairs' zeros into them); rec: the caller's record buffers (the dict
    this returns: counter, ray, w, xyz, off, cnt), which may be longer than rec_cap."""
    origins = f32(origins, "origins", 3)
    dirs = f32(dirs, "dirs", 3)
    z_vals = f32(z_vals, "z_vals").view(-1)
    dev = origins.device
    n_sample = z_vals.numel()
    org_map = None if org_map is None else i32(org_map, "org_map")
    dir_map = None if dir_map is None else i32(dir_map, "dir_map")
    if active is not None:
        active = _req(active, torch.uint8, "active")
    if vis is None:
        vis = torch.empty((n_rays,), dtype=torch.float32, device=dev)
    if oma is None:
        oma = torch.empty((n_rays,), dtype=torch.float32, device=dev) if want_nerfactor else None
    if not want_records:
        rec = None
    elif rec is not None:
        if min(rec["ray"].numel(), rec["w"].numel(), rec["xyz"].shape[0]) < rec_cap or min(rec["off"].numel(), rec["cnt"].numel()) < n_rays:
            raise ValueError("march_secondary: rec buffers smaller than rec_cap records / n_rays rays")
        rec = dict(rec, cap=rec_cap)
    else:
        rec = {
            # [total, written prefix]; `counter`: a caller-owned pair that is already zero on the device
            "counter": counter if counter is not None else torch.zeros((2,), dtype=torch.int32, device=dev),
            "ray": torch.empty((rec_cap,), dtype=torch.int32, device=dev),
            "w": torch.empty((rec_cap,), dtype=torch.float32, device=dev),
            "xyz": torch.empty((rec_cap, 3), dtype=torch.float32, device=dev),
            "off": torch.empty((n_rays,), dtype=torch.int32, device=dev),
            "cnt": rec_cnt if rec_cnt is not None else torch.empty((n_rays,), dtype=torch.int32, device=dev),
            "cap": rec_cap,
        }
    r = rec or {}
    if ray_ids is not None:
        ray_ids = i32(ray_ids, "ray_ids")
    _call("tir_march_secondary_fwd" if ray_ids is None else "tir_march_secondary_ids_fwd",
          C.byref(field), _ptr(origins), _ptr(org_map), _ptr(dirs), _ptr(dir_map), _ptr(active),
          n_rays, int(n_dirs), n_sample, _ptr(z_vals), float(t_stop), _ptr(vis), _ptr(oma),
          _ptr(r.get("counter")), int(rec_cap), _ptr(r.get("ray")), _ptr(r.get("w")), _ptr(r.get("xyz")),
          _ptr(r.get("off")), _ptr(r.get("cnt")), _stats_ptr("tir_march_secondary_fwd", dev),
          *(() if ray_ids is None else (_ptr(ray_ids), _ptr(n_ids_dev))), _stream())
    return vis, oma, rec


def accumulate_records(off, cnt, rec_w, rec_rgb, n_rays):
    out = torch.empty((n_rays, 3), dtype=torch.float32, device=off.device)
    _call("tir_accumulate_records", _ptr(off), _ptr(cnt), _ptr(rec_w), _ptr(rec_rgb), n_rays,
                                       _ptr(out), _stream())
    return out


# ---- shading --------------------------------------------------------------------------------------
def env_sg(lgtSGs, rot, dirs):
    sgs = f32(lgtSGs.detach(), "lgtSGs", 7)
    rot = f32(rot, "light_rotation_matrix").view(-1, 9)
    dirs = f32(dirs, "dirs", 3).view(-1, 3)
    L, D = rot.shape[0], dirs.shape[0]
    out = torch.empty((L, D, 3), dtype=torch.float32, device=dirs.device)
    desc = TirEnvSG(sgs.data_ptr(), rot.data_ptr(), sgs.shape[0], L)
    _call("tir_env_sg_fwd", C.byref(desc), _ptr(dirs), D, _ptr(out), _stream())
    return out


def env_pixel(light_rgbs, H, W, rot, dirs, softplus=True):
    """light_kind == 'pixel': [H*W, 3] raw map parameters -> environment radiance [L, D, 3] (tir_env_pixel_fwd); softplus=False:
    the image as it is (light_kind == 'gt', the data set's probe)."""
    lr = f32(light_rgbs.detach(), "_light_rgbs", 3).view(-1, 3)
    if lr.shape[0] != H * W:
        raise ValueError(f"_light_rgbs: expected {H * W} rows, got {lr.shape[0]}")
    rot = f32(rot, "light_rotation_matrix").view(-1, 9)
    dirs = f32(dirs, "dirs", 3).view(-1, 3)
    L, D = rot.shape[0], dirs.shape[0]
    out = torch.empty((L, D, 3), dtype=torch.float32, device=dirs.device)
    _call("tir_env_pixel_fwd", _ptr(lr), int(H), int(W), _ptr(rot), _ptr(dirs), L, D, int(bool(softplus)), _ptr(out), _stream())
    return out


def env_pixel_bwd(light_rgbs, H, W, rot, dirs, g_env):
    lr = f32(light_rgbs.detach(), "_light_rgbs", 3).view(-1, 3)
    rot = f32(rot, "light_rotation_matrix").view(-1, 9)
    dirs = f32(dirs, "dirs", 3).view(-1, 3)
    g_env = f32(g_env, "g_env", 3)
    L, D = rot.shape[0], dirs.shape[0]
    g = torch.zeros_like(lr)
    _call("tir_env_pixel_bwd", _ptr(lr), int(H), int(W), _ptr(rot), _ptr(dirs), L, D, _ptr(g_env), _ptr(g), _stream())
    return g.view_as(light_rgbs)


def shade_setup(maps, rays, dirs, acc_thres=-1e30):
    maps = f32(maps, "maps", MAP_STRIDE)
    rays = f32(rays, "rays", 6)
    dirs = f32(dirs, "dirs", 3)
    M, D = maps.shape[0], dirs.shape[0]
    surf = torch.empty((M, 3), dtype=torch.float32, device=maps.device)
    active = torch.empty((M, D), dtype=torch.uint8, device=maps.device)
    _call("tir_shade_setup", _ptr(maps), _ptr(rays), _ptr(dirs), M, D, float(acc_thres), _ptr(surf), _ptr(active),
                                _stream())
    return surf, active


def shade_setup_compact(maps, rays, dirs, acc_thres, n_active):
    """shade_setup + compacted active-pair list.  n_active: zeroed int32 device scalar (re-armed by
    shade_integrate_records).  Returns surf, active, pair_ids [M*D], vis [M*D] and rec_cnt [M*D] (zeros at masked pairs)."""
    maps = f32(maps, "maps", MAP_STRIDE)
    rays = f32(rays, "rays", 6)
    dirs = f32(dirs, "dirs", 3)
    M, D = maps.shape[0], dirs.shape[0]
    dev = maps.device
    surf = torch.empty((M, 3), dtype=torch.float32, device=dev)
    active = torch.empty((M, D), dtype=torch.uint8, device=dev)
    pair_ids = torch.empty((M * D,), dtype=torch.int32, device=dev)
    vis = torch.empty((M * D,), dtype=torch.float32, device=dev)
    rec_cnt = torch.empty((M * D,), dtype=torch.int32, device=dev)
    _call("tir_shade_setup_compact", _ptr(maps), _ptr(rays), _ptr(dirs), M, D, float(acc_thres), _ptr(surf), _ptr(active),
          _ptr(pair_ids), _ptr(n_active), _ptr(vis), _ptr(rec_cnt), TUNE["pair_order"], _stream())
    return surf, active, pair_ids, vis, rec_cnt


def shade_integrate(maps, rays, dirs, light_idx, vis, indirect, env, weight_d, equal_area=False,
                    use_srgb=True, acc_thres=-1e30):
    maps = f32(maps, "maps", MAP_STRIDE)
    rays = f32(rays, "rays", 6)
    dirs = f32(dirs, "dirs", 3)
    M, D = maps.shape[0], dirs.shape[0]
    light_idx = i32(light_idx, "light_idx").view(-1)
    vis = f32(vis, "vis")
    env = f32(env, "env", 3)
    if indirect is not None:
        indirect = f32(indirect, "indirect", 3)
    if weight_d is not None:
        weight_d = f32(weight_d, "light_area_weight")
    out = torch.empty((M, 3), dtype=torch.float32, device=maps.device)
    _call("tir_shade_integrate", _ptr(maps), _ptr(rays), _ptr(dirs), _ptr(light_idx), _ptr(vis),
                                    _ptr(indirect), _ptr(env), _ptr(weight_d), M, D, env.shape[0],
                                    int(bool(equal_area)), int(bool(use_srgb)), float(acc_thres), _ptr(out), _stream())
    return out


def shade_integrate_records(maps, rays, dirs, light_idx, vis, rec_off, rec_cnt, rec_w, rec_rgb, env, weight_d,
                            equal_area=False, use_srgb=True, acc_thres=-1e30, reset_counter=None):
    """shade_integrate with the per-ray indirect sum fused in (reads the secondary records directly)."""
    maps = f32(maps, "maps", MAP_STRIDE)
    rays = f32(rays, "rays", 6)
    dirs = f32(dirs, "dirs", 3)
    M, D = maps.shape[0], dirs.shape[0]
    light_idx = i32(light_idx, "light_idx").view(-1)
    env = f32(env, "env", 3)
    if weight_d is not None:
        weight_d = f32(weight_d, "light_area_weight")
    out = torch.empty((M, 3), dtype=torch.float32, device=maps.device)
    _call("tir_shade_integrate_records", _ptr(maps), _ptr(rays), _ptr(dirs), _ptr(light_idx), _ptr(f32(vis, "vis")),
          _ptr(i32(rec_off, "rec_off")), _ptr(i32(rec_cnt, "rec_cnt")), _ptr(f32(rec_w, "rec_w")),
          _ptr(f32(rec_rgb, "rec_rgb", 3)), _ptr(env), _ptr(weight_d), M, D, env.shape[0], int(bool(equal_area)),
          int(bool(use_srgb)), float(acc_thres), _ptr(out), _ptr(reset_counter), _stream())
    return out


def relight_importance(normal, albedo, rough, fresnel, rays_d, light_dir, light_rgb, light_pdf, vis):
    normal, albedo = f32(normal, "normal", 3), f32(albedo, "albedo", 3)
    rough = f32(rough, "roughness").view(-1)
    fresnel, rays_d = f32(fresnel, "fresnel", 3), f32(rays_d, "rays_d", 3)
    light_dir, light_rgb = f32(light_dir, "light_dir", 3), f32(light_rgb, "light_rgb", 3)
    M, Ns = light_dir.shape[0], light_dir.shape[1]
    light_pdf = f32(light_pdf, "light_pdf").view(M, Ns)
    vis = f32(vis, "vis").view(M, Ns)
    out = torch.empty((M, 3), dtype=torch.float32, device=normal.device)
    _call("tir_relight_importance", _ptr(normal), _ptr(albedo), _ptr(rough), _ptr(fresnel), _ptr(rays_d),
                                       _ptr(light_dir), _ptr(light_rgb), _ptr(light_pdf), _ptr(vis), M, Ns,
                                       _ptr(out), _stream())
    return out


def env_sample_setup(row_cdf, col_cdf, env_dir, normal, n_samples, seed, offset):
    """Importance samples of an H x W environment map for every surface point + the cosine mask
    (tir_env_sample_setup).  Returns cell [M, Ns] int32, active [M, Ns] uint8."""
    H, W = col_cdf.shape
    normal = f32(normal, "normal", 3)
    M = normal.shape[0]
    cell = torch.empty((M, n_samples), dtype=torch.int32, device=normal.device)
    active = torch.empty((M, n_samples), dtype=torch.uint8, device=normal.device)
    _call("tir_env_sample_setup", _ptr(f32(row_cdf, "row_cdf")), _ptr(f32(col_cdf, "col_cdf")), H, W,
          _ptr(f32(env_dir, "env_dir", 3)), _ptr(normal), M, int(n_samples), int(seed) & (2 ** 64 - 1),
          int(offset) & (2 ** 64 - 1), _ptr(cell), _ptr(active), _stream())
    return cell, active


def c5_pair_order():
    """How the importance-sampled (point, cell) pairs reach the visibility march: TENSOIR_C5_PAIRS = `binned` (default: the
    compacted list of the unmasked pairs, every 512 consecutive pairs -- one surface point at 512 samples -- ordered by a
    15 x 17 grid of direction bins, tir_env_sample_setup_list), `compact` (the same list without the bins) or `mask` (every
    pair with a uint8 mask, tir_env_sample_setup).  Results do not depend on it (profiles/r04_c5_pair_lists.json).
    Returns (mode, bins, block_pairs); TENSOIR_C5_BINS = `RxC` and TENSOIR_C5_BLOCK_PAIRS override the list's grouping."""
    mode = os.environ.get("TENSOIR_C5_PAIRS", "binned").strip().lower() or "binned"
    if mode not in ("binned", "compact", "mask"):
        raise ValueError(f"TENSOIR_C5_PAIRS={mode!r}: expected binned, compact or mask")
    bins, block = ((15, 17), 512) if mode == "binned" else ((1, 1), 512)
    if os.environ.get("TENSOIR_C5_BINS"):
        bins = tuple(int(v) for v in os.environ["TENSOIR_C5_BINS"].lower().split("x"))
        if len(bins) != 2:
            raise ValueError("TENSOIR_C5_BINS: expected ROWSxCOLS, e.g. 8x8")
    if os.environ.get("TENSOIR_C5_BLOCK_PAIRS"):
        block = int(os.environ["TENSOIR_C5_BLOCK_PAIRS"])
    return mode, bins, block


def cdf_guide_tables(row_cdf, col_cdf):
    """Guide tables of the inverse-CDF search (tir_env_sample_setup_list): for G = the next power of two >= n, entry k of
    a table is the search result for u = k / G -- the first index whose cdf exceeds it, clamped to n - 1.  Built with
    torch.searchsorted on the fp32 tables the kernel searches (k / G is exact in fp32).  Returns (row_guide int32 [Gr + 1],
    col_guide [H, Gc + 2] 16-bit entries packed in pairs into int32 [H, Gc / 2 + 1] (little endian; the last entry pads the
    row to whole words), Gr, Gc), or None when a row has more than 65535 columns or fewer than 2 (Gc + 2 entries would not
    fill whole words; a one-column map needs no search)."""
    H, W = col_cdf.shape
    if W > 65535 or W < 2:
        return None
    gr, gc = 1 << max(0, (H - 1).bit_length()), 1 << max(0, (W - 1).bit_length())
    dev = row_cdf.device
    tr = torch.arange(gr + 1, dtype=torch.float32, device=dev) / gr
    tc = torch.arange(gc + 1, dtype=torch.float32, device=dev) / gc
    rg = torch.searchsorted(row_cdf.contiguous(), tr, right=True).clamp_(max=H - 1).to(torch.int32)
    cg = torch.searchsorted(col_cdf.contiguous(), tc.unsqueeze(0).expand(H, -1).contiguous(), right=True).clamp_(max=W - 1)
    rg[-1], cg[:, -1] = H - 1, W - 1
    cg = torch.cat([cg, cg[:, -1:]], dim=1).to(torch.int32)                      # Gc + 2 entries per row
    packed = (cg[:, 0::2] | (cg[:, 1::2] << 16)).to(torch.int32)                 # two 16-bit entries per word
    return rg.contiguous(), packed.contiguous(), gr, gc


def env_sample_setup_list(row_cdf, col_cdf, env_dir, normal, n_samples, seed, offset, bins=(1, 1), block_pairs=256, guide=None,
                          m_dev=None):
    """tir_env_sample_setup_list[_n]: cells of every (point, sample) + the list of the pairs that pass the cosine mask.
    Returns cell [M, Ns] int32, vis [M, Ns] fp32 (0 where masked, the rest for the march to fill), pair_ids [M*Ns] int32,
    n_active [1] int32 (device).  m_dev (int32 device scalar): only the first min(M, m_dev) points exist."""
    H, W = col_cdf.shape
    normal = f32(normal, "normal", 3)
    M, dev = normal.shape[0], normal.device
    cell = torch.empty((M, n_samples), dtype=torch.int32, device=dev)
    vis = torch.empty((M, n_samples), dtype=torch.float32, device=dev)
    pair_ids = torch.empty((M * n_samples,), dtype=torch.int32, device=dev)
    n_active = torch.zeros((1,), dtype=torch.int32, device=dev)
    stride = int(env_dir.shape[-1])                    # [H*W, 3] directions or the [H*W, 8] records of pack_env_cells
    if stride not in (3, 8):
        raise ValueError(f"env_dir: expected [H*W, 3] directions or [H*W, 8] cell records, got {tuple(env_dir.shape)}")
    _call("tir_env_sample_setup_list_n", _ptr(f32(row_cdf, "row_cdf")), _ptr(f32(col_cdf, "col_cdf")), H, W,
          _ptr(f32(env_dir, "env_dir", stride)), stride, _ptr(normal), M, int(n_samples), int(seed) & (2 ** 64 - 1),
          int(offset) & (2 ** 64 - 1), int(bins[0]), int(bins[1]), int(block_pairs),
          *((None, None, 0, 0) if guide is None else (_ptr(_req(guide[0], torch.int32, "row_guide")),
                                                      _ptr(_req(guide[1], torch.int32, "col_guide")), int(guide[2]), int(guide[3]))),
          _ptr(cell), _ptr(vis), _ptr(pair_ids), _ptr(n_active), _ptr(m_dev), _stream())
    return cell, vis, pair_ids, n_active


def pack_env_cells(env_dir, env_rgb, env_pdf):
    """[H*W, 8] fp32 records {dir.xyz, pdf_return, rgb, 0} of an environment map for tir_relight_importance_cells_packed."""
    d, c, p = f32(env_dir, "env_dir", 3).view(-1, 3), f32(env_rgb, "env_rgb", 3).view(-1, 3), f32(env_pdf, "env_pdf").view(-1, 1)
    return torch.cat([d, p, c, torch.zeros_like(p)], dim=1).contiguous()


def relight_importance_cells(normal, albedo, rough, fresnel, rays_d, cell, env_dir, env_rgb, env_pdf, vis, env_cell=None, m_dev=None):
    """BRDF x radiance x cosine / pdf mean over a point's samples -> sRGB (scripts/relight_importance.py:133-160).  env_cell
    (pack_env_cells of the same three tables): one 32-byte record per sample instead of three gathers; same result.
    m_dev (int32 device scalar, packed form only): only the first min(M, m_dev) points exist (rows beyond: not written)."""
    normal, albedo = f32(normal, "normal", 3), f32(albedo, "albedo", 3)
    rough = f32(rough, "roughness").view(-1)
    fresnel, rays_d = f32(fresnel, "fresnel", 3), f32(rays_d, "rays_d", 3)
    cell = i32(cell, "cell")
    M, Ns = cell.shape
    vis = f32(vis, "vis").view(M, Ns)
    out = torch.empty((M, 3), dtype=torch.float32, device=normal.device)
    if env_cell is not None:
        _call("tir_relight_importance_cells_packed_n", _ptr(normal), _ptr(albedo), _ptr(rough), _ptr(fresnel), _ptr(rays_d), _ptr(cell),
              _ptr(f32(env_cell, "env_cell", 8)), _ptr(vis), M, Ns, _ptr(out), _ptr(m_dev), _stream())
        return out
    if m_dev is not None:
        raise ValueError("relight_importance_cells: a device-side point count needs the packed cell records (env_cell)")
    _call("tir_relight_importance_cells", _ptr(normal), _ptr(albedo), _ptr(rough), _ptr(fresnel), _ptr(rays_d), _ptr(cell),
          _ptr(f32(env_dir, "env_dir", 3)), _ptr(f32(env_rgb, "env_rgb", 3)), _ptr(f32(env_pdf, "env_pdf")), _ptr(vis),
          M, Ns, _ptr(out), _stream())
    return out


def env_mis_setup(row_cdf, col_cdf, env_cell, row_sin, normal, rays_d, rough, n_l, n_b, lobe_select, seed, offset, block_pairs=512,
                  guide=None, m_dev=None, env_pdf=None, buffers=None):
    """tir_env_mis_setup: n_l map-distributed directions (jittered inside their cells) and n_b directions from the BRDF mixture
    (cosine lobe with probability lobe_select, GGX half-vector lobe otherwise) per surface point, N = n_l + n_b.  env_cell: the
    [H*W, 8] records of pack_env_cells, or the [H*W, 3] direction table together with env_pdf [H*W]; row_sin [H]: the sin(theta)
    table hdr_pdf_return was divided by.  Returns dirs [M, N, 3], cell [M, N] int32, pdf_mix [M, N] = (n_l p_l + n_b p_b) / N,
    vis [M, N] (0 where inactive, the rest for the march to fill), pair_ids [M*N] int32, n_active [1] int32 (device).
    m_dev (int32 device scalar): only the first min(M, m_dev) points exist.  buffers: the caller's (dirs, cell, pdf_mix, vis,
    pair_ids) to write into instead of fresh ones."""
    H, W = col_cdf.shape
    normal, rays_d = f32(normal, "normal", 3), f32(rays_d, "rays_d", 3)
    M, dev = normal.shape[0], normal.device
    rough = f32(rough, "roughness").view(-1)
    n_l, n_b = int(n_l), int(n_b)
    N = n_l + n_b
    if n_l < 0 or n_b < 0 or N < 1:
        raise ValueError(f"env_mis_setup: n_l, n_b >= 0 and n_l + n_b >= 1, got {n_l} and {n_b}")
    if rays_d.shape[0] != M or rough.numel() != M:
        raise ValueError(f"env_mis_setup: normal, rays_d and roughness describe the same {M} points")
    stride = int(env_cell.shape[-1])
    if stride not in (3, 8) or env_cell.shape[0] != H * W or (stride == 3 and env_pdf is None):
        raise ValueError(f"env_cell: expected [H*W, 8] cell records or [H*W, 3] directions plus env_pdf, got {tuple(env_cell.shape)}")
    row_sin = f32(row_sin, "row_sin").view(-1)
    if row_sin.numel() != H:
        raise ValueError(f"row_sin: expected {H} rows, got {row_sin.numel()}")
    if buffers is not None:
        dirs, cell, pdf_mix, vis, pair_ids = buffers
        want = ((M, N, 3), torch.float32), ((M, N), torch.int32), ((M, N), torch.float32), ((M, N), torch.float32), ((M * N,), torch.int32)
        for t, (shape, dt) in zip(buffers, want):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"env_mis_setup: buffers are contiguous (dirs, cell, pdf_mix, vis, pair_ids) for {M} points x {N} pairs")
    else:
        dirs = torch.empty((M, N, 3), dtype=torch.float32, device=dev)
        cell = torch.empty((M, N), dtype=torch.int32, device=dev)
        pdf_mix = torch.empty((M, N), dtype=torch.float32, device=dev)
        vis = torch.empty((M, N), dtype=torch.float32, device=dev)
        pair_ids = torch.empty((M * N,), dtype=torch.int32, device=dev)
    n_active = torch.zeros((1,), dtype=torch.int32, device=dev)
    _call("tir_env_mis_setup", _ptr(f32(row_cdf, "row_cdf")), _ptr(f32(col_cdf, "col_cdf")), H, W, _ptr(f32(env_cell, "env_cell", stride)),
          stride, _ptr(None if env_pdf is None else f32(env_pdf, "env_pdf")), _ptr(row_sin), _ptr(normal), _ptr(rays_d), _ptr(rough), M,
          n_l, n_b, float(lobe_select), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(block_pairs),
          *((None, None, 0, 0) if guide is None else (_ptr(_req(guide[0], torch.int32, "row_guide")),
                                                      _ptr(_req(guide[1], torch.int32, "col_guide")), int(guide[2]), int(guide[3]))),
          _ptr(dirs), _ptr(cell), _ptr(pdf_mix), _ptr(vis), _ptr(pair_ids), _ptr(n_active), _ptr(m_dev), _stream())
    return dirs, cell, pdf_mix, vis, pair_ids, n_active


def relight_mis(normal, albedo, rough, fresnel, rays_d, dirs, cell, pdf_mix, env_cell, vis, linear=False, m_dev=None):
    """tir_relight_mis: mean over a point's N pairs of (albedo / pi + GGX) x vis x radiance of the pair's cell x cosine / pdf_mix
    on env_mis_setup's buffers and the [H*W, 8] cell records -> [M, 3], clamped to [0, 1] and sRGB-encoded, or with linear=True
    the raw mean.  m_dev (int32 device scalar): only the first min(M, m_dev) points exist (rows beyond: not written)."""
    normal, albedo = f32(normal, "normal", 3), f32(albedo, "albedo", 3)
    rough = f32(rough, "roughness").view(-1)
    fresnel, rays_d = f32(fresnel, "fresnel", 3), f32(rays_d, "rays_d", 3)
    cell = i32(cell, "cell")
    M, N = cell.shape
    dirs = f32(dirs, "dirs", 3).view(M, N, 3)
    pdf_mix, vis = f32(pdf_mix, "pdf_mix").view(M, N), f32(vis, "vis").view(M, N)
    if normal.shape[0] != M:
        raise ValueError(f"relight_mis: cell has {M} rows, normal {normal.shape[0]}")
    out = torch.empty((M, 3), dtype=torch.float32, device=normal.device)
    _call("tir_relight_mis", _ptr(normal), _ptr(albedo), _ptr(rough), _ptr(fresnel), _ptr(rays_d), _ptr(dirs), _ptr(cell), _ptr(pdf_mix),
          _ptr(f32(env_cell, "env_cell", 8)), _ptr(vis), M, N, int(bool(linear)), _ptr(out), _ptr(m_dev), _stream())
    return out


def env_lookup(env_rgb, dirs):
    """Bilinear lookup of an [H, W, 3] map at [n, 3] directions (tir_env_lookup)."""
    env_rgb = f32(env_rgb, "env_rgb", 3)
    H, W = env_rgb.shape[0], env_rgb.shape[1]
    dirs = f32(dirs, "dirs", 3).view(-1, 3)
    out = torch.empty_like(dirs)
    _call("tir_env_lookup", _ptr(env_rgb), H, W, _ptr(dirs), dirs.shape[0], _ptr(out), _stream())
    return out


def surface_compact(maps, rays, acc_thres=0.5):
    """tir_surface_compact: the acc > acc_thres rows of a chunk's primary maps [B, 20] as compacted surface-point arrays
    (capacity B, ascending row order) -> dict(surf, normal, albedo, rough, fresnel, rays_d, slot [B] int32, n_hit [1] int32)."""
    maps = f32(maps, "maps", MAP_STRIDE)
    rays = f32(rays, "rays", 6)
    B, dev = rays.shape[0], rays.device
    v3 = lambda: torch.empty((B, 3), dtype=torch.float32, device=dev)
    out = {"surf": v3(), "normal": v3(), "albedo": v3(), "rough": torch.empty((B,), dtype=torch.float32, device=dev), "fresnel": v3(),
           "rays_d": v3(), "slot": torch.empty((B,), dtype=torch.int32, device=dev), "n_hit": torch.empty((1,), dtype=torch.int32, device=dev)}
    _call("tir_surface_compact", _ptr(maps), _ptr(rays), B, float(acc_thres), _ptr(out["surf"]), _ptr(out["normal"]), _ptr(out["albedo"]),
          _ptr(out["rough"]), _ptr(out["fresnel"]), _ptr(out["rays_d"]), _ptr(out["slot"]), _ptr(out["n_hit"]), _stream())
    return out


def env_compose(env_rgb, rays, slot, fg_rgb, out, col=0):
    """tir_env_compose: out[:, col:col+3] = the relit colour fg_rgb[slot[i]] of a foreground row, the background lookup of the
    map at the ray direction rays[i, 3:6] otherwise.  out [B, >= col + 3] fp32, written in place."""
    env_rgb = f32(env_rgb, "env_rgb", 3)
    rays = f32(rays, "rays", 6)
    B = rays.shape[0]
    if out.dtype != torch.float32 or not out.is_contiguous() or out.shape[0] != B or out.shape[1] < col + 3:
        raise ValueError("env_compose: out must be a contiguous fp32 [B, >= col + 3] tensor")
    _call("tir_env_compose", _ptr(env_rgb), env_rgb.shape[0], env_rgb.shape[1], C.c_void_p(rays.data_ptr() + 12), 6, B,
          _ptr(i32(slot, "slot")), _ptr(f32(fg_rgb, "fg_rgb", 3)), C.c_void_p(out.data_ptr() + 4 * col), int(out.shape[1]), _stream())
    return out


def ggx_specular(normal, v, l, rough, fresnel):
    normal, v = f32(normal, "normal", 3), f32(v, "pts2c", 3)
    l = f32(l, "pts2l", 3)
    M, D = l.shape[0], l.shape[1]
    rough = f32(rough.expand(M, 3) if rough.shape[-1] == 1 else rough, "roughness", 3)
    fresnel = f32(fresnel.expand(M, 3) if fresnel.shape[-1] == 1 else fresnel, "fresnel", 3)
    out = torch.empty((M, D, 3), dtype=torch.float32, device=l.device)
    _call("tir_ggx_specular", _ptr(normal), _ptr(v), _ptr(l), _ptr(rough), _ptr(fresnel), M, D,
                                 _ptr(out), _stream())
    return out


# ---- training (backward) kernels: SURVEY.md section 8(f)-1 -------------------------------------------
from ._lib import TirFieldGrad  # noqa: E402


def march_primary_train(field: TirField, rays, ray_jitter, n_samples, t_stop):
    """march_primary that also returns the per-sample density sigma [B,S] (needed by the backward)."""
    rays = f32(rays, "rays", 6)
    B, dev = rays.shape[0], rays.device
    if ray_jitter is not None:
        ray_jitter = f32(ray_jitter, "ray_jitter").view(-1)
    weight = torch.empty((B, n_samples), dtype=torch.float32, device=dev)
    sigma = torch.empty((B, n_samples), dtype=torch.float32, device=dev)
    acc = torch.empty((B,), dtype=torch.float32, device=dev)
    depth = torch.empty((B,), dtype=torch.float32, device=dev)
    tend = torch.empty((B,), dtype=torch.float32, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("tir_march_primary_train_fwd", C.byref(field), _ptr(rays), _ptr(ray_jitter), B, n_samples, float(t_stop),
          _ptr(weight), _ptr(sigma), _ptr(acc), _ptr(depth), _ptr(tend), _ptr(cnt), _stream())
    return weight, sigma, acc, depth, tend, cnt


def composite_primary_bwd(rays, offsets, rec_k, rec_w, rgb, brdf, brdf_jit, pred_n, der_n, acc, depth, S,
                          white_bg, is_relight, fixed_fresnel, g_maps):
    rays = f32(rays, "rays", 6)
    g_maps = f32(g_maps, "g_maps", MAP_STRIDE)
    B, dev = rays.shape[0], rays.device
    like = lambda t: None if t is None else torch.empty_like(t)
    g_rgb, g_brdf, g_brdf_jit, g_pred, g_der = like(rgb), like(brdf), like(brdf_jit), like(pred_n), like(der_n)
    g_weight = torch.zeros((B, S), dtype=torch.float32, device=dev)
    g_acc = torch.empty((B,), dtype=torch.float32, device=dev)
    g_depth = torch.empty((B,), dtype=torch.float32, device=dev)
    _call("tir_composite_primary_bwd", _ptr(rays), _ptr(offsets), _ptr(rec_k), _ptr(rec_w), _ptr(rgb), _ptr(brdf),
          _ptr(brdf_jit), _ptr(pred_n), _ptr(der_n), _ptr(acc), _ptr(depth), B, int(S), int(bool(white_bg)),
          int(bool(is_relight)), float(fixed_fresnel), _ptr(g_maps), _ptr(g_rgb), _ptr(g_brdf), _ptr(g_brdf_jit),
          _ptr(g_pred), _ptr(g_der), _ptr(g_weight), _ptr(g_acc), _ptr(g_depth), _stream())
    return g_rgb, g_brdf, g_brdf_jit, g_pred, g_der, g_weight, g_acc, g_depth


def march_primary_bwd(field: TirField, grad: TirFieldGrad, rays, ray_jitter, sigma, weight, g_weight, g_acc, g_depth,
                      want_g_feature=False):
    B, S = weight.shape
    g_feature = torch.empty_like(weight) if want_g_feature else None
    if ray_jitter is not None:
        ray_jitter = f32(ray_jitter, "ray_jitter").view(-1)
    _call("tir_march_primary_bwd", C.byref(field), C.byref(grad), _ptr(f32(rays, "rays", 6)), _ptr(ray_jitter), B, S,
          _ptr(f32(sigma, "sigma")), _ptr(f32(weight, "weight")), _ptr(f32(g_weight, "g_weight")),
          _ptr(f32(g_acc, "g_acc")), _ptr(f32(g_depth, "g_depth")), _ptr(g_feature), _stream())
    return g_feature


def density_grad_bwd(field: TirField, grad: TirFieldGrad, xyz, g_normal):
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    g_normal = f32(g_normal, "g_normal", 3).view(-1, 3)
    _call("tir_density_grad_bwd", C.byref(field), C.byref(grad), _ptr(xyz), _ptr(g_normal), xyz.shape[0], _stream())


def density_feat_grad(field: TirField, xyz, want_feat=True, want_grad=True):
    """compute_densityfeature_with_xyz_grad's feature [n] (border-clamped taps) and its gradient in xyz [n, 3]
    (tir_density_feat_grad_fwd)."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    feat = torch.empty((n,), dtype=torch.float32, device=xyz.device) if want_feat else None
    grad = torch.empty((n, 3), dtype=torch.float32, device=xyz.device) if want_grad else None
    _call("tir_density_feat_grad_fwd", C.byref(field), _ptr(xyz), _ptr(feat), _ptr(grad), n, _stream())
    return feat, grad


def vm_density_bwd(field: TirField, grad: TirFieldGrad, xyz, g_feat):
    """Scatter d loss / d density feature [n] at the points xyz into the density planes / lines (tir_vm_density_bwd)."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    g_feat = f32(g_feat, "g_feat").view(-1)
    _call("tir_vm_density_bwd", C.byref(field), C.byref(grad), _ptr(xyz), _ptr(g_feat), xyz.shape[0], _stream())


def density_feat_bwd(field: TirField, grad, xyz, g_feat, want_xyz=True):
    """Backward of density_feat_grad's feature: parameter scatter into `grad` (None: skipped) and, when want_xyz, the
    coordinate gradient g_feat * d feat / d xyz [n, 3] (tir_density_feat_bwd)."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    g_feat = f32(g_feat, "g_feat").view(-1)
    g_xyz = torch.empty_like(xyz) if want_xyz else None
    _call("tir_density_feat_bwd", C.byref(field), None if grad is None else C.byref(grad), _ptr(xyz), _ptr(g_feat),
          _ptr(g_xyz), xyz.shape[0], _stream())
    return g_xyz


def density_feat_grad_bwd(field: TirField, grad, xyz, v, want_xyz=True):
    """Double backward of density_feat_grad: for cotangents v [n, 3] of d feat / d xyz, the parameter VJP into `grad` (None:
    skipped) and, when want_xyz, the Hessian-vector product [n, 3] (tir_density_feat_grad_bwd)."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    v = f32(v, "v", 3).view(-1, 3)
    g_xyz = torch.empty_like(xyz) if want_xyz else None
    _call("tir_density_feat_grad_bwd", C.byref(field), None if grad is None else C.byref(grad), _ptr(xyz), _ptr(v),
          _ptr(g_xyz), xyz.shape[0], _stream())
    return g_xyz


def vm_app_bwd(field: TirField, grad: TirFieldGrad, xyz, light_idx, idx_map, g_rad, g_int):
    """Scatter d feat into the appearance planes/lines + light rows; returns (y_rad, y_int) [n, 3*Ca]."""
    xyz = f32(xyz, "xyz", 3).view(-1, 3)
    n = xyz.shape[0]
    nch = 3 * field.n_acomp
    g_rad = None if g_rad is None else f32(g_rad, "g_rad")
    g_int = None if g_int is None else f32(g_int, "g_int")
    stride = (g_rad if g_rad is not None else g_int).shape[1]
    y_rad = torch.empty((n, nch), dtype=torch.float32, device=xyz.device) if g_rad is not None else None
    y_int = torch.empty((n, nch), dtype=torch.float32, device=xyz.device) if g_int is not None else None
    if light_idx is not None:
        light_idx = i32(light_idx, "light_idx").view(-1)
    if idx_map is not None:
        idx_map = i32(idx_map, "idx_map").view(-1)
    _call("tir_vm_app_bwd", C.byref(field), C.byref(grad), _ptr(xyz), _ptr(light_idx), _ptr(idx_map), _ptr(g_rad),
          _ptr(g_int), stride, n, _ptr(y_rad), _ptr(y_int), _stream())
    return y_rad, y_int


def mlp_train(m: "PackedMlp", feat, aux, aux_map=None, aux_mod=0, impl=None, n_dev=None):
    """Decoder forward that also returns the hidden activations (h1, h2) [n,128]: split-bf16 matrix cores when the
    product's decoder mode is bf16x3 (default), exact fp32 MFMA otherwise.  n_dev: device-side row count (rows past
    it are left unwritten)."""
    impl = impl or MLP_IMPL
    feat = f32(feat, "feat")
    aux = f32(aux, "aux", 3)
    n = feat.shape[0]
    if aux_map is not None:
        aux_map = i32(aux_map, "aux_map").view(-1)
    out = torch.empty((n, m.out_dim), dtype=torch.float32, device=feat.device)
    h1 = torch.empty((n, 128), dtype=torch.float32, device=feat.device)
    h2 = torch.empty((n, 128), dtype=torch.float32, device=feat.device)
    _call("tir_mlp_train_fwd_bf16x3" if impl == "bf16x3" else "tir_mlp_train_fwd", C.byref(m.desc), _ptr(feat),
          feat.shape[1], _ptr(aux), _ptr(aux_map), int(aux_mod), _ptr(out), _ptr(h1), _ptr(h2), n, _ptr(n_dev), _stream())
    return out, h1, h2


def mlp_inputs(m: "PackedMlp", feat, aux, aux_map=None, aux_mod=0):
    feat = f32(feat, "feat")
    aux = f32(aux, "aux", 3)
    n = feat.shape[0]
    if aux_map is not None:
        aux_map = i32(aux_map, "aux_map").view(-1)
    x = torch.empty((n, 160), dtype=torch.float32, device=feat.device)
    _call("tir_mlp_inputs", C.byref(m.desc), _ptr(feat), feat.shape[1], _ptr(aux), _ptr(aux_map), int(aux_mod),
          _ptr(x), n, _stream())
    return x


def pack_mlp_bwd(w0, w1, w2, feat_dim, pe):
    ws = [f32(t.detach(), "mlp weight") for t in (w0, w1, w2)]
    hidden, out_dim = w1.shape[0], w2.shape[0]
    n = lib().tir_mlp_bwd_packed_floats(feat_dim, pe, hidden, out_dim)
    if n < 0:
        check(int(n), "tir_mlp_bwd_packed_floats")
    packed = torch.empty((int(n),), dtype=torch.float32, device=w0.device)
    _call("tir_pack_mlp_bwd", *[_ptr(t) for t in ws], feat_dim, pe, hidden, out_dim, _ptr(packed), _stream())
    return packed


def mlp_bwd(m: "PackedMlp", packed_bwd, feat, out, g_out, h1, h2, impl=None):
    """Backward-data of one decoder (g_feat, dz1, dz2, dz3): split-bf16 matrix cores when the product's decoder mode
    is bf16x3 (default), exact fp32 MFMA otherwise."""
    impl = impl or MLP_IMPL
    feat = f32(feat, "feat")
    n = feat.shape[0]
    dev = feat.device
    g_feat = torch.empty((n, FEAT_STRIDE), dtype=torch.float32, device=dev)
    dz1 = torch.empty((n, 128), dtype=torch.float32, device=dev)
    dz2 = torch.empty((n, 128), dtype=torch.float32, device=dev)
    dz3 = torch.empty((n, 4), dtype=torch.float32, device=dev)
    _call("tir_mlp_bwd_bf16x3" if impl == "bf16x3" else "tir_mlp_bwd", C.byref(m.desc), _ptr(packed_bwd), _ptr(feat),
          feat.shape[1], _ptr(f32(out, "out")),
          _ptr(f32(g_out, "g_out")), _ptr(h1), _ptr(h2), n, _ptr(g_feat), _ptr(dz1), _ptr(dz2), _ptr(dz3), _stream())
    return g_feat, dz1, dz2, dz3


def mlp_bwd_multi(jobs):
    """Backward-data of up to four decoder invocations over the same rows in one launch (tir_mlp_bwd_multi_bf16x3).
    jobs: list of (PackedMlp, packed_bwd, feat [n, FEAT_STRIDE], out, g_out, h1, h2); returns [(g_feat, dz1, dz2, dz3)]."""
    k = len(jobs)
    n = jobs[0][2].shape[0]
    dev = jobs[0][2].device
    res, cols = [], [[] for _ in range(11)]
    for m, pb, feat, out, g_out, h1, h2 in jobs:
        feat = f32(feat, "feat")
        if feat.shape[0] != n or feat.shape[1] != FEAT_STRIDE:
            raise ValueError(f"mlp_bwd_multi: every job needs [n, {FEAT_STRIDE}] feature rows")
        g_feat = torch.empty((n, FEAT_STRIDE), dtype=torch.float32, device=dev)
        dz1 = torch.empty((n, 128), dtype=torch.float32, device=dev)
        dz2 = torch.empty((n, 128), dtype=torch.float32, device=dev)
        dz3 = torch.empty((n, 4), dtype=torch.float32, device=dev)
        res.append((g_feat, dz1, dz2, dz3))
        for c, t in zip(cols, (pb, feat, f32(out, "out"), f32(g_out, "g_out"), h1, h2, g_feat, dz1, dz2, dz3)):
            c.append(t)
    arr = lambda ts: (C.c_void_p * k)(*[t.data_ptr() for t in ts])
    descs = (C.POINTER(TirMlp) * k)(*[C.pointer(j[0].desc) for j in jobs])
    _call("tir_mlp_bwd_multi_bf16x3", descs, arr(cols[0]), arr(cols[1]), FEAT_STRIDE, arr(cols[2]), arr(cols[3]), arr(cols[4]),
          arr(cols[5]), k, n, arr(cols[6]), arr(cols[7]), arr(cols[8]), arr(cols[9]), _stream())
    _KEEP_ALIVE = cols          # noqa: F841  (operands stay referenced until the launch is queued)
    return res


def gemm_tn_small(pairs, M, N, C_out):
    """C_out[M, N] += sum over the (A, B) pairs of A[:, :M]^T @ B[:, :N], M <= 32, N <= 160, every pair over the same number of
    rows (tir_gemm_tn_small_bf16x3: the basis-matrix gradient of several appearance gathers in one launch)."""
    k = len(pairs)
    As = [f32(a, "A") for a, _ in pairs]
    Bs = [f32(b, "B") for _, b in pairs]
    n = As[0].shape[0]
    if any(a.shape[0] != n or b.shape[0] != n or a.shape[1] != As[0].shape[1] or b.shape[1] != Bs[0].shape[1] for a, b in zip(As, Bs)):
        raise ValueError("gemm_tn_small: every pair needs the same row count and strides")
    arr = lambda ts: (C.c_void_p * k)(*[t.data_ptr() for t in ts])
    _call("tir_gemm_tn_small_bf16x3", arr(As), As[0].shape[1], int(M), arr(Bs), Bs[0].shape[1], int(N), k, n, _ptr(C_out),
          C_out.shape[1], _stream())
    _KEEP_ALIVE = (As, Bs)          # noqa: F841
    return C_out


def mlp_wgrad_multi(jobs):
    """Weight gradients of up to four decoder invocations over the same rows in ONE launch (tir_mlp_wgrad_multi): no
    materialised input rows, no per-layer GEMM launches.  jobs: list of (dz1, dz2, dz3, h1, h2, feat [n, stride >= 27; 32 = FEAT_STRIDE takes the LDS-staged kernel], aux,
    aux_map or None, dW0 [128,150], db0 [128], dW1 [128,128], db1 [128], dW2 [4,128], db2 [4]); the six outputs are
    accumulated into (zero them first; two jobs may name the same outputs)."""
    k = len(jobs)
    n = jobs[0][0].shape[0]
    cols = [[] for _ in range(14)]
    null_map = True
    for job in jobs:
        dz1, dz2, dz3, h1, h2, feat, aux, aux_map, dW0, db0, dW1, db1, dW2, db2 = job
        feat = f32(feat, "feat")
        if feat.shape[0] != n or feat.shape[1] < 27 or feat.shape[1] != jobs[0][5].shape[1]:
            raise ValueError("mlp_wgrad_multi: every job needs [n, stride >= 27] feature rows of one common stride")
        for t, shape, name in ((dz1, (n, 128), "dz1"), (dz2, (n, 128), "dz2"), (dz3, (n, 4), "dz3"), (h1, (n, 128), "h1"),
                               (h2, (n, 128), "h2"), (dW0, (128, 150), "dW0"), (db0, (128,), "db0"), (dW1, (128, 128), "dW1"),
                               (db1, (128,), "db1"), (dW2, (4, 128), "dW2"), (db2, (4,), "db2")):
            if tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError(f"mlp_wgrad_multi: {name} must be contiguous fp32 {shape}, got {tuple(t.shape)}")
        aux = f32(aux, "aux", 3)
        if aux_map is not None:
            aux_map = i32(aux_map, "aux_map")
            null_map = False
        for c, t in zip(cols, (dz1, dz2, dz3, h1, h2, feat, aux, aux_map, dW0, db0, dW1, db1, dW2, db2)):
            c.append(t)
    arr = lambda ts: (C.c_void_p * k)(*[(0 if t is None else t.data_ptr()) for t in ts])
    _call("tir_mlp_wgrad_multi", arr(cols[0]), arr(cols[1]), arr(cols[2]), arr(cols[3]), arr(cols[4]), arr(cols[5]), int(jobs[0][5].shape[1]),
          arr(cols[6]), (None if null_map else arr(cols[7])), arr(cols[8]), arr(cols[9]), arr(cols[10]), arr(cols[11]),
          arr(cols[12]), arr(cols[13]), k, n, TUNE["wgrad_blocks"], _stream())
    _KEEP_ALIVE = cols          # noqa: F841  (operands stay referenced until the launch is queued)


def gemm_tn(A, M, B, N, C_out, ones_col=False, impl=None, bias_out=None):
    """C_out[M, N(+1)] += A[:, :M]^T @ B[:, :N]  (+ column N = A^T 1, or bias_out[M] += A^T 1 when given).  Split-bf16
    matrix cores when the product's decoder mode is bf16x3 (default), exact fp32 MFMA otherwise."""
    impl = impl or MLP_IMPL
    A, B = f32(A, "A"), f32(B, "B")
    n = A.shape[0]
    if B.shape[0] != n:
        raise ValueError("gemm_tn: row counts differ")
    _call("tir_gemm_tn_bf16x3" if impl == "bf16x3" else "tir_gemm_tn", _ptr(A), A.shape[1], int(M), _ptr(B), B.shape[1], int(N), int(bool(ones_col)), n,
          _ptr(C_out), C_out.shape[1], _ptr(bias_out), _stream())
    return C_out


def adam_step(entries, beta1, beta2, eps):
    """tir_adam_step over entries (p, g, m, v, lr, bias_correction1, bias_correction2); the four tensors of an entry are
    dense with the same element order (tensoir_amd.optim.Adam checks)."""
    n = len(entries)
    PA, FA, LA = C.c_void_p * n, C.c_float * n, C.c_int64 * n
    _call("tir_adam_step", n, PA(*[e[0].data_ptr() for e in entries]), PA(*[e[1].data_ptr() for e in entries]),
          PA(*[e[2].data_ptr() for e in entries]), PA(*[e[3].data_ptr() for e in entries]),
          LA(*[e[0].numel() for e in entries]), FA(*[e[4] for e in entries]), FA(*[e[5] for e in entries]),
          FA(*[e[6] for e in entries]), float(beta1), float(beta2), float(eps), _stream())


def adam_tables(triples):
    """The argument tables of tir_adam_step for a FIXED parameter list [(p, m, v)]: parameter / moment pointers and element counts
    filled in, gradient pointers and the three per-step float columns left for the caller (tensoir_amd.optim.Adam._fast_step).
    -> (p, m, v, numel, g, lr, bias_correction1, bias_correction2) ctypes arrays."""
    n = len(triples)
    PA, FA, LA = C.c_void_p * n, C.c_float * n, C.c_int64 * n
    return (PA(*[t[0].data_ptr() for t in triples]), PA(*[t[1].data_ptr() for t in triples]), PA(*[t[2].data_ptr() for t in triples]),
            LA(*[t[0].numel() for t in triples]), PA(), FA(), FA(), FA())


def adam_step_tables(n, tables, beta1, beta2, eps):
    """tir_adam_step on prepared tables (adam_tables; the library copies them into the launch: they can be refilled at once)."""
    p, m, v, numel, g, lr, b1, b2 = tables
    _call("tir_adam_step", n, p, g, m, v, numel, lr, b1, b2, float(beta1), float(beta2), float(eps), _stream())


def shade_integrate_bwd(maps, rays, dirs, light_idx, vis, indirect, env, weight_d, equal_area, use_srgb, acc_thres,
                        g_out):
    maps = f32(maps, "maps", MAP_STRIDE)
    M, D = maps.shape[0], dirs.shape[0]
    g_maps = torch.empty_like(maps)
    g_env = torch.zeros_like(env)
    _call("tir_shade_integrate_bwd", _ptr(maps), _ptr(f32(rays, "rays", 6)), _ptr(f32(dirs, "dirs", 3)),
          _ptr(i32(light_idx, "light_idx").view(-1)), _ptr(f32(vis, "vis")),
          _ptr(None if indirect is None else f32(indirect, "indirect", 3)), _ptr(f32(env, "env", 3)),
          _ptr(None if weight_d is None else f32(weight_d, "light_area_weight")), M, D, env.shape[0],
          int(bool(equal_area)), int(bool(use_srgb)), float(acc_thres), _ptr(f32(g_out, "g_out", 3)), _ptr(g_maps),
          _ptr(g_env), _stream())
    return g_maps, g_env


def env_sg_bwd(lgtSGs, rot, dirs, g_env):
    sgs = f32(lgtSGs.detach(), "lgtSGs", 7)
    rot = f32(rot, "light_rotation_matrix").view(-1, 9)
    dirs = f32(dirs, "dirs", 3).view(-1, 3)
    g = torch.zeros_like(sgs)
    desc = TirEnvSG(sgs.data_ptr(), rot.data_ptr(), sgs.shape[0], rot.shape[0])
    _call("tir_env_sg_bwd", C.byref(desc), _ptr(dirs), dirs.shape[0], _ptr(f32(g_env, "g_env", 3)), _ptr(g), _stream())
    return g


def marching_cubes(vol, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """Marching cubes of a dense lattice vol [gx, gy, gz] (tir_mc_count + tir_mc_emit; contract: include/tensoir_hip.h).
    -> (verts [V, 3] f32, faces [F, 3] i32, normals [V, 3] f32), all on vol's device.  Vertex i of edge (p, axis) lies at
    origin + (idx(p) + t e_axis) * spacing; faces wind so that their right-hand normal points from inside (value > level)
    to outside.  The totals are read back once (8 bytes, one sync): the output size depends on the data.  An empty surface
    gives zero-row tensors."""
    vol = f32(vol, "vol")
    if vol.dim() != 3:
        raise ValueError(f"vol: expected [gx, gy, gz], got {tuple(vol.shape)}")
    gx, gy, gz = vol.shape
    sp = [float(s) for s in spacing]
    org = [float(o) for o in origin]
    if len(sp) != 3 or len(org) != 3:
        raise ValueError("spacing and origin take three values each")
    nb = int(lib().tir_mc_blocks(gx, gy, gz))
    if nb < 0:
        check(nb, "tir_mc_blocks")
    dev = vol.device
    counts = torch.empty((2, nb), dtype=torch.int32, device=dev)
    offsets = torch.empty((2, nb + 1), dtype=torch.int32, device=dev)
    _call("tir_mc_count", _ptr(vol), gx, gy, gz, float(level), _ptr(counts), _ptr(offsets), _stream())
    n_verts, n_faces = [int(x) for x in offsets[:, nb].cpu()]
    verts = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    vbase = torch.empty((gx * gy * gz,), dtype=torch.int32, device=dev) if n_verts else None
    _call("tir_mc_emit", _ptr(vol), gx, gy, gz, float(level), *sp, *org, _ptr(offsets), n_verts, n_faces, _ptr(vbase),
          _ptr(verts if n_verts else None), _ptr(normals if n_verts else None), _ptr(faces if n_faces else None), _stream())
    return verts, faces, normals


def _lattice(vol, name="vol"):
    vol = f32(vol, name)
    if vol.dim() != 3:
        raise ValueError(f"{name}: expected [gx, gy, gz], got {tuple(vol.shape)}")
    return vol


def label_components(vol, level, connectivity=6):
    """Connected components of {vol > level} on a dense lattice vol [gx, gy, gz] (tir_ccl_label + tir_ccl_table; contract:
    include/tensoir_hip.h).  connectivity 6 (faces) or 26 (faces, edges, corners).
    -> (labels [gx, gy, gz] int32: -1 outside, else the smallest linear index of the point's component,
        table {"roots" [K] int32 ascending, "sizes" [K] int32 voxel counts, "boxes" [K, 6] int32 inclusive (x0, y0, z0, x1, y1,
        z1)}), all on vol's device.  K is read back once (4 bytes, one sync); K = 0 gives zero-row tensors."""
    vol = _lattice(vol)
    if connectivity not in (6, 26):
        raise ValueError(f"connectivity: 6 or 26, not {connectivity!r}")
    gx, gy, gz = vol.shape
    nb = int(lib().tir_ccl_blocks(gx, gy, gz))
    if nb < 0:
        check(nb, "tir_ccl_blocks")
    dev = vol.device
    labels = torch.empty((gx, gy, gz), dtype=torch.int32, device=dev)
    counts = torch.empty((nb,), dtype=torch.int32, device=dev)
    offsets = torch.empty((nb + 1,), dtype=torch.int32, device=dev)
    _call("tir_ccl_label", _ptr(vol), gx, gy, gz, float(level), int(connectivity), _ptr(labels), _ptr(counts), _ptr(offsets),
          _stream())
    K = int(offsets[nb].item())
    roots = torch.empty((K,), dtype=torch.int32, device=dev)
    sizes = torch.empty((K,), dtype=torch.int32, device=dev)
    boxes = torch.empty((K, 6), dtype=torch.int32, device=dev)
    _call("tir_ccl_table", _ptr(labels), gx, gy, gz, _ptr(offsets), K, _ptr(roots if K else None), _ptr(sizes if K else None),
          _ptr(boxes if K else None), _stream())
    return labels, {"roots": roots, "sizes": sizes, "boxes": boxes}


def keep_components(vol, labels, table, keep, fill=0.0, level=None):
    """tir_ccl_filter: a new lattice equal to vol where the point is outside or its component is kept (keep [K] bool, in the
    table's order), `fill` elsewhere.  level (optional): the level `labels` was made at -- fill must not exceed it, so that a
    removed point is an outside point of the result; without it the call checks fill <= fill only (nothing)."""
    vol = _lattice(vol)
    labels = i32(labels, "labels")
    if labels.shape != vol.shape or labels.device != vol.device:
        raise ValueError("labels: expected the shape and device of vol")
    roots = i32(table["roots"], "table['roots']").view(-1)
    K = roots.shape[0]
    keep = torch.as_tensor(keep)
    if keep.dtype != torch.bool:
        raise TypeError(f"keep: expected torch.bool, got {keep.dtype}")
    keep = keep.to(vol.device).contiguous().view(-1)          # a [K] flag row: the selection is a host policy (mesh.py)
    if keep.shape[0] != K:
        raise ValueError(f"keep: expected [{K}] flags, got {tuple(keep.shape)}")
    gx, gy, gz = vol.shape
    out = torch.empty_like(vol)
    _call("tir_ccl_filter", _ptr(vol), _ptr(labels), gx, gy, gz, float(fill if level is None else level), _ptr(roots if K else None),
          _ptr(keep if K else None), K, float(fill), _ptr(out), _stream())
    return out


SIMPLIFY_ACC = _K["TIR_SIMPLIFY_ACC"]
_SIMPLIFY_ERRORS = ((_K["TIR_SIMPLIFY_ERR_FACE_INDEX"], "a face index lies outside [0, V)"),
                    (_K["TIR_SIMPLIFY_ERR_FACE_EXTENT"], "a face edge is longer than 4 cells along an axis (or not finite)"),
                    (_K["TIR_SIMPLIFY_ERR_VERTEX"], "a vertex lies more than 3.5 cells outside the lattice of cells (or is not finite)"))


def simplify_mesh(verts, faces, cell, origin=(0.0, 0.0, 0.0), dims=None, reg=1e-2):
    """Quadric vertex clustering (tir_simplify_count + tir_simplify_emit; the definition: include/tensoir_hip.h).  verts [V, 3]
    f32 and faces [F, 3] i32 on the GPU; cell: the cluster's edge (one value or three), origin: the corner of cell (0, 0, 0),
    dims: cells per axis -- None takes floor(max((v - origin) / cell)) + 1 per axis, one extra reduction and read-back.
    -> (verts' [V', 3] f32, faces' [F', 3] i32, normals' [V', 3] f32, cell_of_vertex [V] i32), all on verts' device: one vertex
    per occupied cell in ascending cell order, placed where the summed plane quadrics of the cell's faces are smallest
    (regularised toward the mean of its vertices by `reg`, clamped to the cell); faces that collapse are dropped, the others
    keep order and winding.  Two calls give identical bits.  The two totals and an error word are read back once (16 bytes,
    one sync); a face index outside [0, V), or a face / vertex beyond the extent the fixed-point sums are scaled for, raises."""
    verts = f32(verts, "verts", 3).view(-1, 3)
    faces = i32(faces, "faces").view(-1, 3)
    dev = verts.device
    if faces.device != dev:
        raise ValueError("faces: expected the device of verts")
    V, F = verts.shape[0], faces.shape[0]
    cl = [float(cell)] * 3 if isinstance(cell, (int, float)) else [float(c) for c in cell]
    org = [float(o) for o in origin]
    if len(cl) != 3 or len(org) != 3:
        raise ValueError("cell takes one or three values, origin three")
    if dims is None:
        if V and all(c > 0 for c in cl):
            q = (verts - torch.tensor(org, dtype=torch.float32, device=dev)) / torch.tensor(cl, dtype=torch.float32, device=dev)
            top = torch.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0).amax(0).floor().clamp(0, 2.0 ** 31 - 256).cpu()
            dims = [int(t) + 1 for t in top]
        else:
            dims = [1, 1, 1]
    dm = [int(d) for d in dims]
    if len(dm) != 3:
        raise ValueError("dims takes three values")
    c_cell, c_org = (C.c_float * 3)(*cl), (C.c_float * 3)(*org)
    c_dims = (C.c_int32 * 3)(*[max(min(d, 2 ** 31 - 1), -1) for d in dm])
    n_slots = dm[0] * dm[1] * dm[2]
    if min(dm) < 1 or n_slots > 2 ** 31 - 1 or min(cl) <= 0:
        # the library words the refusal: it validates these on the host, before it looks at any buffer
        check(lib().tir_simplify_count(None, V, None, F, c_cell, c_org, c_dims, None, None, None, None, None, None),
              "tir_simplify_count")
    nbs, nbf = int(lib().tir_simplify_blocks(n_slots)), int(lib().tir_simplify_blocks(F))
    slots = torch.empty((n_slots,), dtype=torch.int32, device=dev)
    counts = torch.empty((max(nbs + nbf, 1),), dtype=torch.int32, device=dev)
    offsets = torch.empty((nbs + nbf + 2,), dtype=torch.int32, device=dev)
    status = torch.empty((4,), dtype=torch.int32, device=dev)
    cov = torch.empty((V,), dtype=torch.int32, device=dev)
    _call("tir_simplify_count", _ptr(verts if V else None), V, _ptr(faces if F else None), F, c_cell, c_org, c_dims, _ptr(slots),
          _ptr(cov if V else None), _ptr(counts), _ptr(offsets), _ptr(status), _stream())
    n_out, n_faces, err, _ = [int(x) for x in status.cpu()]
    if err:
        raise _lib.TensoirHipError("simplify_mesh: " + "; ".join(msg for bit, msg in _SIMPLIFY_ERRORS if err & bit))
    del slots
    out_v = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
    out_n = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    acc = torch.empty((n_out, SIMPLIFY_ACC), dtype=torch.int64, device=dev) if n_out else None
    keys = torch.empty((n_out,), dtype=torch.int32, device=dev) if n_out else None
    _call("tir_simplify_emit", _ptr(verts if V else None), V, _ptr(faces if F else None), F, c_cell, c_org, c_dims, float(reg),
          _ptr(cov if V else None), _ptr(offsets), n_out, n_faces, _ptr(acc), _ptr(keys), _ptr(out_v if n_out else None),
          _ptr(out_n if n_out else None), _ptr(out_f if n_faces else None), _stream())
    return out_v, out_f, out_n, cov


# ---- surface distance between meshes (tir_distance.hip) ------------------------------
DISTANCE_MAX_DIM = _K["TIR_DISTANCE_MAX_DIM"]
DISTANCE_CELL_FACTOR = 2.0
_DISTANCE_FACE_INDEX = "a face index lies outside [0, V)"


def _mesh_args(verts, faces):
    verts = f32(verts, "verts", 3).view(-1, 3)
    faces = i32(faces, "faces").view(-1, 3)
    if faces.device != verts.device:
        raise ValueError("faces: expected the device of verts")
    return verts, faces


def sample_surface(verts, faces, n, seed=0):
    """n area-weighted, stratified samples of a mesh's surface (tir_mesh_sample_cdf + tir_mesh_sample; the definition, hash
    included: include/tensoir_hip.h).  verts [V, 3] f32 and faces [F, 3] i32 on the GPU -> (points [n, 3] f32, face [n] i32) on
    verts' device, samples in face order.  The weights are quantised to integers and summed as integers, so the face of every
    sample is the same on every run and on every device order; faces of integer weight 0 (zero area among them) get no sample.
    One 32-byte read-back (total, error word, statistics; one sync).  A face index outside [0, V) raises TensoirHipError
    ("face index"), a mesh without any area TensoirHipError ("degenerate"); an empty `faces` with n > 0 raises ValueError."""
    verts, faces = _mesh_args(verts, faces)
    n, seed = int(n), int(seed)
    if n < 0:
        raise ValueError("sample_surface: n >= 0")
    if not 0 <= seed < 2 ** 64:
        raise ValueError("sample_surface: seed is an unsigned 64-bit integer")
    V, F = verts.shape[0], faces.shape[0]
    dev = verts.device
    if n > 0 and F == 0:
        raise ValueError("sample_surface: a mesh without faces has no surface to sample")
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return points, face
    nb = int(lib().tir_distance_blocks(F))
    cdf = torch.empty((F,), dtype=torch.int64, device=dev)
    sums = torch.empty((max(nb, 1),), dtype=torch.int64, device=dev)
    status = torch.zeros((4,), dtype=torch.int64, device=dev)
    _call("tir_mesh_sample_cdf", _ptr(verts if V else None), V, _ptr(faces), F, _ptr(cdf), _ptr(sums), _ptr(status), _stream())
    total, err, _, _ = [int(x) for x in status.cpu()]
    if err & _K["TIR_DISTANCE_ERR_FACE_INDEX"]:
        raise _lib.TensoirHipError("sample_surface: " + _DISTANCE_FACE_INDEX)
    if total <= 0:
        raise _lib.TensoirHipError("sample_surface: every face is degenerate (no area to sample)")
    _call("tir_mesh_sample", _ptr(verts), V, _ptr(faces), F, _ptr(cdf), n, seed, _ptr(points), _ptr(face), _stream())
    return points, face


def _grid_triplet(x, name, kind):
    vals = [kind(x)] * 3 if isinstance(x, (int, float)) else [kind(v) for v in x]
    if len(vals) != 3:
        raise ValueError(f"{name} takes one or three values")
    return vals


def _face_grid_count(verts, faces, cell, origin, dims):
    V, F = verts.shape[0], faces.shape[0]
    c_cell, c_org = (C.c_float * 3)(*cell), (C.c_float * 3)(*origin)
    c_dims = (C.c_int32 * 3)(*[max(min(d, 2 ** 31 - 1), -1) for d in dims])
    status = torch.zeros((4,), dtype=torch.int64, device=verts.device)      # (F = 0 returns before any device work)
    # (the library words the refusal of cell <= 0 and of dims beyond the limit: it validates them on the host first)
    _call("tir_face_grid_count", _ptr(verts if V else None), V, _ptr(faces if F else None), F, c_cell, c_org, c_dims, _ptr(status),
          _stream())
    pairs, err, degenerate, listed = [int(x) for x in status.cpu()]
    if err & _K["TIR_DISTANCE_ERR_FACE_INDEX"]:
        raise _lib.TensoirHipError("face_grid: " + _DISTANCE_FACE_INDEX)
    return pairs, degenerate, listed, (c_cell, c_org, c_dims)


def face_grid(verts, faces, cell=None, max_pairs=None, *, dims=None, origin=None):
    """A uniform grid over a mesh's faces for point_mesh_distance (tir_face_grid_count + tir_face_grid_fill; the definition:
    include/tensoir_hip.h).  verts [V, 3] f32, faces [F, 3] i32 on the GPU.  Every non-degenerate face is listed in every cell
    its bounding box overlaps; a face without area (|cross|^2 == 0 in fp64) or with a non-finite corner is listed nowhere and
    counted in "degenerate".  origin (default): the smallest finite vertex coordinates; dims (default): floor(extent / cell) + 1.
    cell (one value or three): the cell edge.  cell=None chooses it: DISTANCE_CELL_FACTOR x the mean edge of the faces' finite
    bounding boxes (all three axes together), raised per axis to extent / DISTANCE_MAX_DIM so that dims stay <= 256, and then
    doubled (all axes) until the pairs fit max_pairs; with dims given and no cell, cell = extent / dims per axis.
    max_pairs: the most (face, cell) pairs the grid may hold, default max(16 F, 2^20) (at most 2^31 - 1).  A total above it
    with an explicit cell is REFUSED, TensoirHipError ("pairs", with the true total) -- never truncated.  A grid of 1 x 1 x 1
    lists every face in its one cell: the brute-force path.
    -> {"cell", "origin", "dims": host lists, "cursor" [cells] i32 (the end of every cell's list), "pairs" [P] i32 (face
    indices; the order inside a cell may differ between runs, no result of point_mesh_distance depends on it), "n_pairs",
    "degenerate", "listed", "n_faces", "n_verts", "bounds" [6] f32 on the device (the box of the finite vertices, padded by
    2^-16 max(max |coordinate|, largest extent): what ray_mesh clips its rays to)}.  One small read-back for the bounding box
    (and the mean edge), then one 32-byte read-back (pair total, error word, statistics) per cell edge tried; a face index outside [0, V) raises
    TensoirHipError ("face index")."""
    verts, faces = _mesh_args(verts, faces)
    V, F = verts.shape[0], faces.shape[0]
    dev = verts.device
    limit = 2 ** 31 - 1
    max_pairs = min(max(16 * F, 2 ** 20), limit) if max_pairs is None else int(max_pairs)
    if not 0 <= max_pairs <= limit:
        raise ValueError(f"face_grid: max_pairs in 0 .. {limit}")
    lo = hi = None
    bounds = torch.zeros((6,), dtype=torch.float32, device=dev)
    if V:
        fin = torch.isfinite(verts)
        big = torch.finfo(torch.float32).max
        lo_t = torch.where(fin, verts, torch.full_like(verts, big)).amin(0)
        hi_t = torch.where(fin, verts, torch.full_like(verts, -big)).amax(0)
        pad = torch.maximum(torch.maximum(lo_t.abs(), hi_t.abs()).amax(), (hi_t - lo_t).amax()) * (2.0 ** -16)
        bounds = torch.cat([lo_t - pad, hi_t + pad])                  # (stays on the device: ray_mesh clips its rays to it)
        mean_edge = None
        if cell is None and dims is None and F:
            idx = faces.long().clamp(0, V - 1)
            tri = verts[idx]                                          # [F, 3, 3]
            ext = tri.amax(1) - tri.amin(1)
            ok = torch.isfinite(ext)
            mean_edge = torch.where(ok, ext, torch.zeros_like(ext)).double().sum() / ok.sum().clamp(min=1)
        host = torch.cat([lo_t.double(), hi_t.double(), torch.zeros(1, dtype=torch.float64, device=dev) if mean_edge is None
                          else mean_edge.reshape(1)]).cpu().tolist()
        lo, hi, mean_edge = host[:3], host[3:6], host[6]
        if any(l > h for l, h in zip(lo, hi)):
            lo = hi = None
    if lo is None:
        lo, hi, mean_edge = [0.0] * 3, [0.0] * 3, 0.0
    org = lo if origin is None else _grid_triplet(origin, "origin", float)
    extent = [max(h - o, 0.0) for h, o in zip(hi, org)]
    auto = cell is None and dims is None
    if cell is not None:
        cl = _grid_triplet(cell, "cell", float)
    elif dims is not None:
        dm = _grid_triplet(dims, "dims", int)
        cl = [e / max(d, 1) * (1.0 + 1e-6) if e > 0 else 1.0 for e, d in zip(extent, dm)]
    else:
        base = DISTANCE_CELL_FACTOR * mean_edge if mean_edge > 0 else max(max(extent), 1.0)
        cl = [max(base, e / DISTANCE_MAX_DIM * (1.0 + 1e-6)) for e in extent]
    while True:
        if dims is not None:
            dm = _grid_triplet(dims, "dims", int)
        elif auto:
            dm = [min(int(e / c) + 1, DISTANCE_MAX_DIM) for e, c in zip(extent, cl)]
        else:
            dm = [int(min(e / c, 2.0 ** 31 - 2)) + 1 if c > 0 else 1 for e, c in zip(extent, cl)]
        pairs, degenerate, listed, cargs = _face_grid_count(verts, faces, cl, org, dm)
        if pairs <= max_pairs:
            break
        if not auto or max(dm) == 1:
            raise _lib.TensoirHipError(f"face_grid: the grid needs {pairs} (face, cell) pairs, max_pairs allows {max_pairs}; "
                                       "nothing is truncated -- take a larger cell or raise max_pairs")
        cl = [2.0 * c for c in cl]
    n_cells = dm[0] * dm[1] * dm[2]
    nbc = int(lib().tir_distance_blocks(n_cells))
    cursor = torch.empty((n_cells,), dtype=torch.int32, device=dev) if pairs else torch.zeros((n_cells,), dtype=torch.int32, device=dev)
    counts = torch.empty((max(nbc, 1),), dtype=torch.int32, device=dev)
    offsets = torch.empty((nbc + 1,), dtype=torch.int32, device=dev)
    plist = torch.empty((pairs,), dtype=torch.int32, device=dev)
    _call("tir_face_grid_fill", _ptr(verts if V else None), V, _ptr(faces if F else None), F, *cargs, pairs, _ptr(cursor), _ptr(counts),
          _ptr(offsets), _ptr(plist if pairs else None), _stream())
    return {"cell": [float(c) for c in cargs[0]], "origin": [float(o) for o in cargs[1]], "dims": dm, "cursor": cursor, "pairs": plist,
            "n_pairs": pairs, "degenerate": degenerate, "listed": listed, "n_faces": F, "n_verts": V, "bounds": bounds}


def point_mesh_distance(points, verts, faces, grid=None, closest=False, tested=False):
    """The exact unsigned distance of points to a mesh (tir_point_mesh_distance; the definition: include/tensoir_hip.h).
    points [n, 3] f32, verts [V, 3] f32, faces [F, 3] i32 on one GPU; grid: face_grid(verts, faces) of THIS mesh (None builds
    the default one).  -> (dist [n] f32, face [n] i32), plus closest [n, 3] f32 with closest=True and the number of
    point-triangle tests [n] i32 with tested=True.  The closest point per triangle is found in fp64 (seven regions), the search
    walks shells of grid cells and stops only when no unvisited cell can hold a face as near; ties go to the smaller face index:
    the outputs are bit-identical for every grid over the same faces and on every run.  A mesh without a listed face gives
    dist = +inf and face = -1, a non-finite point dist = NaN and face = -1.  No read-back when a grid is handed in."""
    verts, faces = _mesh_args(verts, faces)
    points = f32(points, "points", 3).view(-1, 3)
    dev = verts.device
    if points.device != dev:
        raise ValueError("points: expected the device of verts")
    if grid is None:
        grid = face_grid(verts, faces)
    V, F, n = verts.shape[0], faces.shape[0], points.shape[0]
    if grid["n_faces"] != F or grid["n_verts"] != V or grid["cursor"].device != dev:
        raise ValueError("grid: not a face_grid of this mesh")
    dist = torch.empty((n,), dtype=torch.float32, device=dev)
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    cl = torch.empty((n, 3), dtype=torch.float32, device=dev) if closest else None
    nt = torch.empty((n,), dtype=torch.int32, device=dev) if tested else None
    P = grid["n_pairs"]
    _call("tir_point_mesh_distance", _ptr(points if n else None), n, _ptr(verts if V else None), V, _ptr(faces if F else None), F,
          (C.c_float * 3)(*grid["cell"]), (C.c_float * 3)(*grid["origin"]), (C.c_int32 * 3)(*grid["dims"]), _ptr(grid["cursor"]),
          _ptr(grid["pairs"] if P else None), P, _ptr(dist if n else None), _ptr(face if n else None),
          _ptr(cl if closest and n else None), _ptr(nt if tested and n else None), _stream())
    return (dist, face) + ((cl,) if closest else ()) + ((nt,) if tested else ())


RAY_MODES = {"closest": _K["TIR_RAY_CLOSEST"], "count": _K["TIR_RAY_COUNT"], "any": _K["TIR_RAY_ANY"]}
RAY_GRAZED, RAY_INVALID = _K["TIR_RAY_FLAG_GRAZED"], _K["TIR_RAY_FLAG_INVALID"]
# TIR_RAY_INSIDE_DIRECTIONS: the three fixed directions of mesh_inside (fp32)
MESH_INSIDE_DIRECTIONS = ((0.5345225, 0.2672612, 0.8017837), (-0.6882472, 0.6246950, -0.3692745), (0.1825742, -0.9128709, -0.3651484))


def _ray_grid(verts, faces, grid, what):
    if grid is None:
        grid = face_grid(verts, faces)
    if grid["n_faces"] != faces.shape[0] or grid["n_verts"] != verts.shape[0] or grid["cursor"].device != verts.device \
            or "bounds" not in grid:
        raise ValueError(f"{what}: grid is not a face_grid of this mesh")
    return grid


def ray_mesh(origins, dirs, verts, faces, grid=None, mode="closest", trange=None, bary=False, count=False, flags=False, tested=False):
    """Rays against a mesh (tir_ray_mesh; the ray-triangle rule, the traversal and the modes: include/tensoir_hip.h).
    origins, dirs [n, 3] f32 (a direction need not be unit: t is in units of |d|), trange [n, 2] f32 or None ([0, +inf]), verts
    [V, 3] f32, faces [F, 3] i32, all on one GPU; grid: face_grid(verts, faces) of THIS mesh (None builds the default one).
    mode "closest" / "count" -> (t [n] f32, face [n] i32) followed, in this order, by bary [n, 2] f32 (weights of the face's
    second and third corner), count [n] i32, flags [n] i32 (RAY_GRAZED, RAY_INVALID) and tested [n] i32 for the options that are
    set.  A miss: t = +inf, face = -1, bary = NaN.  "count" counts every accepted hit exactly and walks the whole ray; "closest"
    may stop early, its count is 0 or 1 and its grazed flag speaks of the reported hit only.  mode "any" -> (hit [n] bool),
    followed by flags and tested if set; bary and count are refused.  Everything but `tested` is bit-identical for every grid
    over the same faces and on every run.  An invalid ray (non-finite, d == 0, NaN range or t0 > t1): t = NaN, face = -1,
    count = 0, flags = RAY_INVALID.  No read-back when a grid is handed in."""
    if mode not in RAY_MODES:
        raise ValueError(f"ray_mesh: mode is one of {sorted(RAY_MODES)}")
    any_mode = mode == "any"
    if any_mode and (bary or count):
        raise ValueError('ray_mesh: mode "any" reports no bary and no count (which face is met first depends on the grid)')
    verts, faces = _mesh_args(verts, faces)
    origins = f32(origins, "origins", 3).view(-1, 3)
    dirs = f32(dirs, "dirs", 3).view(-1, 3)
    dev = verts.device
    n = origins.shape[0]
    if dirs.shape[0] != n:
        raise ValueError("dirs: one direction per origin")
    if trange is not None:
        trange = f32(trange, "trange", 2).view(-1, 2)
        if trange.shape[0] != n:
            raise ValueError("trange: one [t0, t1] per ray")
    if any(x.device != dev for x in (origins, dirs) + (() if trange is None else (trange,))):
        raise ValueError("origins, dirs, trange: expected the device of verts")
    grid = _ray_grid(verts, faces, grid, "ray_mesh")
    V, F, P = verts.shape[0], faces.shape[0], grid["n_pairs"]

    def buf(want, dtype, *shape):
        return torch.empty(shape, dtype=dtype, device=dev) if want else None
    t, face = buf(not any_mode, torch.float32, n), buf(not any_mode, torch.int32, n)
    bc, fl, nt = buf(bary, torch.float32, n, 2), buf(flags, torch.int32, n), buf(tested, torch.int32, n)
    cnt = buf(count or any_mode, torch.int32, n)
    _call("tir_ray_mesh", _ptr(origins if n else None), _ptr(dirs if n else None), _ptr(trange if n and trange is not None else None), n,
          _ptr(verts if V else None), V, _ptr(faces if F else None), F, (C.c_float * 3)(*grid["cell"]), (C.c_float * 3)(*grid["origin"]),
          (C.c_int32 * 3)(*grid["dims"]), _ptr(grid["cursor"]), _ptr(grid["pairs"] if P else None), P, _ptr(grid["bounds"]),
          RAY_MODES[mode], *[_ptr(x if x is not None and n else None) for x in (t, face, bc, cnt, fl, nt)], _stream())
    if any_mode:
        return (cnt != 0,) + ((fl,) if flags else ()) + ((nt,) if tested else ())
    return (t, face) + ((bc,) if bary else ()) + ((cnt,) if count else ()) + ((fl,) if flags else ()) + ((nt,) if tested else ())


def mesh_inside(points, verts, faces, grid=None):
    """Which points lie inside a closed mesh: the parity of the hits of three "count" rays of ray_mesh from each point along
    MESH_INSIDE_DIRECTIONS over [0, +inf].  -> (inside [n] bool = at least two odd counts, votes [n] uint8 = the odd counts, 0 .. 3,
    grazed [n] bool = a ray passed exactly through an edge or a vertex, whose crossing may have been counted twice).  Parity
    means inside only for a mesh whose every directed edge occurs as often as its reverse (mesh.topology's "closed").  A
    non-finite point gets no vote.  Bit-identical for every grid and run; no read-back when a grid is handed in."""
    verts, faces = _mesh_args(verts, faces)
    points = f32(points, "points", 3).view(-1, 3)
    if points.device != verts.device:
        raise ValueError("points: expected the device of verts")
    grid = _ray_grid(verts, faces, grid, "mesh_inside")
    n = points.shape[0]
    votes = torch.zeros((n,), dtype=torch.uint8, device=verts.device)
    grazed = torch.zeros((n,), dtype=torch.bool, device=verts.device)
    for d in MESH_INSIDE_DIRECTIONS:
        dirs = torch.tensor(d, dtype=torch.float32, device=verts.device).expand(n, 3).contiguous()
        _, _, cnt, fl = ray_mesh(points, dirs, verts, faces, grid, mode="count", count=True, flags=True)
        votes += (cnt & 1).to(torch.uint8)
        grazed |= (fl & RAY_GRAZED) != 0
    return votes >= 2, votes, grazed


# ---- per-point bake (tensoir_amd/bake.py) ---------------------------------------------------------
BAKE_ROW = _K["TIR_BAKE_ROW"]


def bake_composite(off, cnt, rec_w, rec_xyz, rec_brdf, rec_normal, origins, dirs, fallback_normal, aabb):
    """tir_bake_composite: the records of the inward march (march_secondary's off / cnt / w / xyz, one ray per point) and their
    decoder outputs rec_brdf [A, 4], rec_normal [A, 3] -> rows [N, BAKE_ROW] = albedo 3, roughness, normal 3, coverage,
    surface 3, depth, 0 x 4 (contract: include/tensoir_hip.h).  aabb: the model's [2, 3] box (host or device)."""
    origins = f32(origins, "origins", 3).view(-1, 3)
    n = origins.shape[0]
    dirs = f32(dirs, "dirs", 3).view(-1, 3)
    fallback_normal = f32(fallback_normal, "fallback_normal", 3).view(-1, 3)
    off, cnt = i32(off, "ray_rec_off").view(-1), i32(cnt, "ray_rec_cnt").view(-1)
    rec_w = f32(rec_w, "rec_w").view(-1)
    a = rec_w.shape[0]
    rec_xyz, rec_brdf, rec_normal = f32(rec_xyz, "rec_xyz", 3), f32(rec_brdf, "rec_brdf", 4), f32(rec_normal, "rec_normal", 3)
    if not (dirs.shape[0] == fallback_normal.shape[0] == off.numel() == cnt.numel() == n):
        raise ValueError("origins, dirs, fallback_normal, ray_rec_off and ray_rec_cnt take one row per point")
    if not (rec_xyz.shape[0] == rec_brdf.shape[0] == rec_normal.shape[0] == a):
        raise ValueError("rec_w, rec_xyz, rec_brdf and rec_normal take one row per record")
    box = (C.c_float * 6)(*[float(v) for v in torch.as_tensor(aabb).detach().reshape(-1).tolist()])
    rows = torch.empty((n, BAKE_ROW), dtype=torch.float32, device=origins.device)
    _call("tir_bake_composite", _ptr(off), _ptr(cnt), _ptr(rec_w), _ptr(rec_xyz), _ptr(rec_brdf), _ptr(rec_normal), _ptr(origins),
          _ptr(dirs), _ptr(fallback_normal), box, n, a, _ptr(rows), _stream())
    return rows


def irradiance_integrate(rows, dirs, vis, env, weight_d, light_idx):
    """tir_irradiance_integrate: rows [M, BAKE_ROW] of bake_composite, dirs [D, 3], vis [M, D], env [L, D, 3], weight_d [D],
    light_idx [M] int32 -> [M, 4] = ambient occlusion, direct irradiance rgb."""
    rows = f32(rows, "rows", BAKE_ROW).view(-1, BAKE_ROW)
    dirs = f32(dirs, "dirs", 3).view(-1, 3)
    M, D = rows.shape[0], dirs.shape[0]
    vis = f32(vis, "vis")
    env = f32(env, "env", 3)
    weight_d = f32(weight_d, "light_area_weight").view(-1)
    light_idx = i32(light_idx, "light_idx").view(-1)
    if D == 0 or env.dim() != 3 or env.shape[1] != D or weight_d.numel() != D or vis.numel() != M * D or light_idx.numel() != M:
        raise ValueError(f"expected vis [{M}, {D}], env [L, {D}, 3], weight_d [{D}], light_idx [{M}]")
    out = torch.empty((M, 4), dtype=torch.float32, device=rows.device)
    _call("tir_irradiance_integrate", _ptr(rows), _ptr(dirs), _ptr(vis), _ptr(env), _ptr(weight_d), _ptr(light_idx), M, D,
          env.shape[0], _ptr(out), _stream())
    return out


# ---- per-triangle texture atlas (tensoir_amd/mesh.py: bake_atlas, export_textured) -----------------
ATLAS_MIN_T = 6
ATLAS_MAX_SIZE = 8192


def atlas_layout(F, size):
    """The atlas of F faces in a size x size image (contract: include/tensoir_hip.h, tir_atlas_*) -> (cols, T): cols x cols
    square cells of T x T texels, two faces per cell.  Host arithmetic only.  ValueError when size is not an integer in
    6 .. 8192 or leaves a cell fewer than 6 texels per side (the message names the smallest size that works)."""
    import math
    import numbers
    if isinstance(size, bool) or not isinstance(size, numbers.Integral) or not ATLAS_MIN_T <= size <= ATLAS_MAX_SIZE:
        raise ValueError(f"size: expected an integer in {ATLAS_MIN_T} .. {ATLAS_MAX_SIZE}, not {size!r}")
    if int(F) < 0:
        raise ValueError(f"the number of faces must not be negative, got {F}")
    n_cells = (int(F) + 1) // 2
    cols = math.isqrt(n_cells - 1) + 1 if n_cells > 0 else 1          # ceil(sqrt(n_cells))
    T = int(size) // cols
    if T < ATLAS_MIN_T:
        raise ValueError(f"size {size} leaves {T} texels per cell side: {F} faces need a size of at least {ATLAS_MIN_T * cols}")
    return cols, T


def _atlas_mesh(verts, normals, faces):
    verts = f32(verts, "verts", 3).view(-1, 3)
    normals = f32(normals, "normals", 3).view(-1, 3)
    faces = i32(faces, "faces").view(-1, 3)
    if normals.shape != verts.shape or normals.device != verts.device or faces.device != verts.device:
        raise ValueError("verts and normals take one row per vertex, and faces lives on their device")
    return verts, normals, faces


def _atlas_status(status, what):
    if int(status.item()):
        raise _lib.TensoirHipError(f"{what}: a face index lies outside [0, V)")


def atlas_corners(verts, normals, faces, size, cols, T):
    """tir_atlas_corners: the unwelded mesh of the atlas -> (pos [3F, 3], nrm [3F, 3], tan [3F, 4], uv [3F, 2]) f32 on verts'
    device; pos / nrm are bit copies of verts / normals [faces].  One 4-byte read-back (the error word)."""
    verts, normals, faces = _atlas_mesh(verts, normals, faces)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    pos, nrm, uv = (torch.empty((3 * F, k), dtype=torch.float32, device=dev) for k in (3, 3, 2))
    tan = torch.empty((3 * F, 4), dtype=torch.float32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    data = lambda t: _ptr(t if F else None)
    _call("tir_atlas_corners", data(verts), V, data(normals), data(faces), F, int(size), int(cols), int(T), data(pos), data(nrm),
          data(tan), data(uv), _ptr(status), _stream())
    _atlas_status(status, "atlas_corners")
    return pos, nrm, tan, uv


def atlas_texels(verts, normals, faces, size, cols, T):
    """tir_atlas_texels: where the bake samples the surface, for the ceil(F / 2) * T * T texels of the used cells in cell-major
    order -> (point [N, 3] f32, outward [N, 3] f32 unit, face [N] i32), in the coordinates of verts / normals."""
    verts, normals, faces = _atlas_mesh(verts, normals, faces)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    N = ((F + 1) // 2) * int(T) * int(T)
    point = torch.empty((N, 3), dtype=torch.float32, device=dev)
    outward = torch.empty((N, 3), dtype=torch.float32, device=dev)
    face = torch.empty((N,), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    data = lambda t: _ptr(t if F else None)
    _call("tir_atlas_texels", data(verts), V, data(normals), data(faces), F, int(size), int(cols), int(T), data(point),
          data(outward), data(face), _ptr(status), _stream())
    _atlas_status(status, "atlas_texels")
    return point, outward, face


def atlas_pack(verts, normals, faces, size, cols, T, albedo, roughness, normal, coverage, irradiance=None, ao=None):
    """tir_atlas_pack: the per-texel bake results (cell-major, as atlas_texels orders them) -> (base, orm, normal) images
    [size, size, 4] uint8 in image order.  irradiance given: the base colour is the Lambertian radiance under it
    (color="diffuse"); ao None: the occlusion channel is 255."""
    verts, normals, faces = _atlas_mesh(verts, normals, faces)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    size, T = int(size), int(T)
    N = ((F + 1) // 2) * T * T
    albedo, normal = f32(albedo, "albedo", 3).view(-1, 3), f32(normal, "normal", 3).view(-1, 3)
    roughness, coverage = f32(roughness, "roughness").view(-1), f32(coverage, "coverage").view(-1)
    rows = [albedo.shape[0], normal.shape[0], roughness.shape[0], coverage.shape[0]]
    if irradiance is not None:
        irradiance = f32(irradiance, "irradiance", 3).view(-1, 3)
        rows.append(irradiance.shape[0])
    if ao is not None:
        ao = f32(ao, "ao").view(-1)
        rows.append(ao.shape[0])
    if any(r != N for r in rows):
        raise ValueError(f"the per-texel inputs take {N} rows (ceil(F / 2) * T * T), got {rows}")
    images = [torch.empty((size, size, 4), dtype=torch.uint8, device=dev) for _ in range(3)] if 0 < size <= ATLAS_MAX_SIZE else \
        [torch.empty((1,), dtype=torch.uint8, device=dev)] * 3             # the library words the refusal of such a size
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    data = lambda t: _ptr(t if F else None)
    _call("tir_atlas_pack", data(verts), V, data(normals), data(faces), F, size, int(cols), T, data(albedo),
          _ptr(irradiance if F else None), data(roughness), _ptr(ao if F else None), data(normal), data(coverage),
          _ptr(images[0]), _ptr(images[1]), _ptr(images[2]), _ptr(status), _stream())
    _atlas_status(status, "atlas_pack")
    if F == 0:                                                             # nothing was launched: every texel is unowned
        for img, rgba in zip(images, ((0, 0, 0, 255), (0, 0, 0, 255), (128, 128, 255, 255))):
            img.copy_(torch.tensor(rgba, dtype=torch.uint8, device=dev).expand(size, size, 4))
    return tuple(images)


# ---- z-buffer rasteriser of the exported mesh (tensoir_amd/raster.py) -------------------
RASTER_MAX_SIDE = _K["TIR_RASTER_MAX_SIDE"]
RASTER_ROW = _K["TIR_RASTER_ROW"]
RASTER_DROPS = ("index", "near", "guard", "nonfinite")     # the order of tir_raster_project's status counts


def _raster_camera(c2w, focal):
    c = torch.as_tensor(c2w).detach().to("cpu", torch.float32).reshape(-1)
    if c.numel() != 12:
        raise ValueError("c2w: expected a [3, 4] camera-to-world matrix")
    return (C.c_float * 12)(*c.tolist()), float(focal)


def raster_project(pos, c2w, focal, H, W, faces=None, near=1e-3):
    """tir_raster_project: pos [3F, 3] (unwelded; or verts [V, 3] with faces [F, 3] int32) f32 on the device, c2w [3, 4] and focal
    on the host -> (rows [3F, 4] int32 = {sx, sy, bits(1 / Z), flags}, drops = {"index", "near", "guard", "nonfinite": faces
    dropped}).  TensoirHipError when a face index lies outside [0, V).  One 16-byte read-back (the counts)."""
    pos = f32(pos, "pos", 3).view(-1, 3)
    dev, V = pos.device, pos.shape[0]
    if faces is not None:
        faces = i32(faces, "faces").view(-1, 3)
        if faces.device != dev:
            raise ValueError("faces lives on pos' device")
        F = faces.shape[0]
    else:
        if V % 3:
            raise ValueError("an unwelded mesh takes three rows of pos per face")
        F = V // 3
    cam, focal = _raster_camera(c2w, focal)
    rows = torch.empty((3 * F, 4), dtype=torch.int32, device=dev)
    status = torch.zeros((4,), dtype=torch.int32, device=dev)
    data = lambda t: _ptr(t if F else None)
    _call("tir_raster_project", data(pos), V, data(faces), F, cam, focal, int(W), int(H), float(near), data(rows), _ptr(status),
          _stream())
    drops = dict(zip(RASTER_DROPS, (int(x) for x in status.tolist())))
    if drops["index"]:
        raise _lib.TensoirHipError("raster_project: a face index lies outside [0, V)")
    return rows, drops


def raster_cover(rows, H, W, cull=True):
    """tir_raster_cover: the projected corners -> keys [H, W] int64 holding the uint64 (bits(1 / Z) << 32) | (0xFFFFFFFF - face)
    of the nearest fragment, 0 where the pixel is empty."""
    rows = i32(rows, "rows").view(-1, 4)
    F = rows.shape[0] // 3
    big = 0 < int(W) <= RASTER_MAX_SIDE and 0 < int(H) <= RASTER_MAX_SIDE
    keys = torch.empty((int(H), int(W)) if big else (1, 1), dtype=torch.int64, device=rows.device)   # the library words the refusal
    work = torch.empty((F + 1,), dtype=torch.int32, device=rows.device)
    _call("tir_raster_cover", _ptr(rows if F else None), F, int(W), int(H), int(bool(cull)), _ptr(keys), _ptr(work), _stream())
    return keys


def raster_resolve(rows, keys):
    """tir_raster_resolve -> (face [H, W] int32, -1 where empty; bary [H, W, 2] f32 = (b1, b2), perspective-correct; zc [H, W] f32,
    the camera-space depth Z), views of one [H, W, 4] buffer."""
    rows = i32(rows, "rows").view(-1, 4)
    keys = _req(keys, torch.int64, "keys")
    H, W = keys.shape
    F = rows.shape[0] // 3
    out = torch.empty((H, W, 4), dtype=torch.int32, device=rows.device)
    _call("tir_raster_resolve", _ptr(rows if F else None), F, _ptr(keys), W, H, _ptr(out), _stream())
    return out[..., 0], out[..., 1:3].view(torch.float32), out[..., 3].view(torch.float32), out


def raster_shade(pix, nrm, tan=None, uv=None, images=None, raw=False):
    """tir_raster_shade: pix [H, W, 4] (raster_resolve's buffer), the per-corner nrm [3F, 3], tan [3F, 4], uv [3F, 2] and
    images = (base, orm, normal) [S, S, 4] uint8 on the device -> [H, W, 12] f32 rows {albedo 3, roughness, ao, normal 3,
    coverage, 0, 0, 0}.  images None: geometry only (normal = the interpolated unit nrm)."""
    pix = _req(pix, torch.int32, "pix", 4)
    H, W = pix.shape[:2]
    nrm = f32(nrm, "nrm", 3).view(-1, 3)
    F = nrm.shape[0] // 3
    size, ptrs = 0, [None] * 5
    if images is not None:
        tan, uv = f32(tan, "tan", 4).view(-1, 4), f32(uv, "uv", 2).view(-1, 2)
        images = [_req(im, torch.uint8, "images", 4) for im in images]
        size = images[0].shape[0]
        if tan.shape[0] != 3 * F or uv.shape[0] != 3 * F or len(images) != 3 or any(tuple(im.shape) != (size, size, 4) for im in images):
            raise ValueError("tan [3F, 4], uv [3F, 2] and three [S, S, 4] images are expected")
        ptrs = [_ptr(tan if F else None), _ptr(uv if F else None)] + [_ptr(im) for im in images]
    out = torch.empty((H, W, RASTER_ROW), dtype=torch.float32, device=pix.device)
    _call("tir_raster_shade", _ptr(pix), F, _ptr(nrm if F else None), *ptrs, int(size), int(bool(raw)), W, H, _ptr(out), _stream())
    return out


# ---- lighting of the exported asset (tensoir_amd/raster.py) -----------------------------
LIGHT_OCCLUSION = _K["TIR_LIGHT_OCCLUSION"]
LIGHT_SRGB = _K["TIR_LIGHT_SRGB"]


def env_row_weights(H, W):
    """float64 [H]: the exact solid angle of one texel of row i of an H x W equirectangular map,
    (2 pi / W) * 2 sin(pi (i + 0.5) / H) * sin(pi / (2 H)); W times their sum is 4 pi."""
    i = torch.arange(int(H), dtype=torch.float64)
    return (2.0 * math.pi / int(W)) * 2.0 * torch.sin(math.pi * (i + 0.5) / int(H)) * math.sin(math.pi / (2.0 * int(H)))


def env_cells(hdr, h, w):
    """tir_env_cells: an [H, W, 3] map on the device -> [h * w, 8] light cells {dir, solid angle, rgb, 0}, each the solid-angle
    weighted mean of its (H / h) x (W / w) texels.  ValueError unless H and W are multiples of h and w."""
    hdr = f32(hdr, "hdr", 3)
    if hdr.dim() != 3:
        raise ValueError("env_cells: an [H, W, 3] map is expected")
    H, W, h, w = hdr.shape[0], hdr.shape[1], int(h), int(w)
    if h < 1 or w < 1 or H % h or W % w:
        raise ValueError(f"env_cells: the map's sides {H} x {W} must be multiples of the cell grid's {h} x {w}")
    row_w = to_device(env_row_weights(H, W).to(torch.float32), hdr.device)
    cells = torch.empty((h * w, 8), dtype=torch.float32, device=hdr.device)
    _call("tir_env_cells", _ptr(hdr), H, W, _ptr(row_w), h, w, _ptr(cells), _stream())
    return cells


def light_gbuffer(gbuf, view, cells, fresnel=0.04, occlusion=True, srgb=False):
    """tir_light_gbuffer: gbuf [..., 12] (raster_shade's rows), view [..., 3] (surface to eye), cells [D, 8] (env_cells) ->
    [..., 4] = {r, g, b, coverage}: the environment integrated against albedo / pi + GGX over the cells above the stored normal's
    horizon, times ao with occlusion, tone-mapped with srgb.  Rows without coverage are zeros."""
    gbuf, view, cells = f32(gbuf, "gbuf", RASTER_ROW), f32(view, "view", 3), f32(cells, "cells", 8).view(-1, 8)
    if gbuf.shape[:-1] != view.shape[:-1]:
        raise ValueError("light_gbuffer: gbuf and view take one row per pixel")
    if cells.shape[0] < 1:
        raise ValueError("light_gbuffer: at least one light cell")
    out = torch.empty(gbuf.shape[:-1] + (4,), dtype=torch.float32, device=gbuf.device)
    flags = (LIGHT_OCCLUSION if occlusion else 0) | (LIGHT_SRGB if srgb else 0)
    _call("tir_light_gbuffer", _ptr(gbuf), _ptr(view), _ptr(cells), gbuf.numel() // RASTER_ROW, cells.shape[0], float(fresnel), flags,
          _ptr(out), _stream())
    return out


# ---- shadows of the exported asset: one orthographic z-buffer per light cell (tensoir_amd/raster.py) --------------
SHADOW_MAX_SIDE = _K["TIR_SHADOW_MAX_SIDE"]
SHADOW_WORK_CAP = 1 << 16      # listed (cell, face) pairs of shadow_maps' workgroup pass; any value gives the same maps


def shadow_frames_f64(dirs, centre, radius, S):
    """shadow_frames' host arithmetic: dirs [D, 3] (any length), centre [3], radius, S -> float64 numpy [D, 12]."""
    L = np.asarray(dirs, np.float64).reshape(-1, 3)
    c = np.asarray(centre, np.float64).reshape(3)
    r, S = float(radius), int(S)
    if L.shape[0] < 1 or not r > 0 or not np.isfinite(r) or S < 1:
        raise ValueError("shadow_frames: at least one cell, a positive finite radius and S >= 1")
    n = np.linalg.norm(L, axis=1, keepdims=True)
    if not (np.isfinite(n).all() and (n > 0).all()):
        raise ValueError("shadow_frames: every cell needs a finite direction of non-zero length")
    L = L / n
    u = np.cross(np.eye(3)[np.argmin(np.abs(L), axis=1)], L)         # argmin takes the first of equal values
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(L, u)
    g = S / (2.0 * r)
    return np.concatenate([g * u, (S / 2.0 - g * (u @ c))[:, None], g * v, (S / 2.0 - g * (v @ c))[:, None],
                           L / (4.0 * r), (0.5 - (L @ c) / (4.0 * r))[:, None]], 1)


def shadow_frames(cells, centre, radius, S):
    """The orthographic frame of every light cell round the sphere (centre, radius) for S x S maps -> frames [D, 12] f32 on cells'
    device, formed in float64 on the host (shadow_frames_f64) and rounded once.  With L = cells[d, 0:3] normalised, a the axis with
    the smallest |L_a| (lowest index on ties), u = normalize(e_a x L), v = L x u, g = S / (2 r): row d is {g u, S/2 - g u.c, g v,
    S/2 - g v.c, L / (4 r), 0.5 - L.c / (4 r)} (include/tensoir_hip.h).  One read-back of the D directions."""
    cells = f32(cells, "cells", 8).view(-1, 8)
    fr = shadow_frames_f64(cells[:, 0:3].detach().to("cpu", torch.float64).numpy(), centre, radius, S)
    return to_device(torch.from_numpy(fr.astype(np.float32)), cells.device).contiguous()


def _shadow_inputs(frames, maps=None):
    frames = f32(frames, "frames", 12).view(-1, 12)
    if frames.shape[0] < 1:
        raise ValueError("frames: at least one light cell")
    if maps is None:
        return frames
    maps = _req(maps, torch.int32, "maps")
    if maps.dim() != 3 or maps.shape[0] != frames.shape[0] or maps.shape[1] != maps.shape[2] or maps.shape[1] < 1:
        raise ValueError("maps: expected [D, S, S] int32 (shadow_maps), one map per row of frames")
    return frames, maps


def shadow_maps(pos, frames, S, faces=None, work_cap=SHADOW_WORK_CAP):
    """tir_shadow_maps: pos [3F, 3] (unwelded; or verts [V, 3] with faces [F, 3] int32) f32 and frames [D, 12] (shadow_frames) on
    the device -> (maps [D, S, S] int32 holding the uint32 bits(w) of the surface nearest to each cell's light, 0 where the texel
    is empty; drops = {"index", "near", "guard", "nonfinite": dropped (cell, face) PAIRS}, near always 0).  work_cap: how many
    pairs with large boxes the workgroup pass may take; the maps do not depend on it.  One 32-byte read-back (the counts)."""
    pos = f32(pos, "pos", 3).view(-1, 3)
    frames = _shadow_inputs(frames)
    dev, V, D, S, work_cap = pos.device, pos.shape[0], frames.shape[0], int(S), int(work_cap)
    if faces is not None:
        faces = i32(faces, "faces").view(-1, 3)
        if faces.device != dev:
            raise ValueError("faces lives on pos' device")
        F = faces.shape[0]
    else:
        if V % 3:
            raise ValueError("an unwelded mesh takes three rows of pos per face")
        F = V // 3
    if frames.device != dev or work_cap < 0:
        raise ValueError("shadow_maps: frames lives on pos' device, and work_cap >= 0")
    ok = 0 < S <= SHADOW_MAX_SIDE
    maps = torch.empty((D, S, S) if ok else (1, 1, 1), dtype=torch.int32, device=dev)          # the library words the refusal
    work = torch.empty((2 + 2 * work_cap,), dtype=torch.int32, device=dev)
    status = torch.zeros((4,), dtype=torch.int64, device=dev)
    data = lambda t: _ptr(t if F else None)
    _call("tir_shadow_maps", data(pos), V, data(faces), F, _ptr(frames), D, S, _ptr(maps), _ptr(work), work_cap, _ptr(status), _stream())
    return maps, dict(zip(RASTER_DROPS, (int(x) for x in status.tolist())))


def shadow_lookup(pts, nrm, cells, frames, maps, bias=(0.0, 0.0)):
    """tir_shadow_lookup: pts, nrm [M, 3], cells [D, 8], frames [D, 12], maps [D, S, S] -> vis [M, D] uint8: 0 = the pair does not
    contribute (n.L <= 1e-6), 1 = shadowed, 2 = lit, by the visibility rule tir_light_gbuffer_shadowed applies (nearest texel;
    bias = (const, slope) in texels)."""
    pts, nrm, cells = f32(pts, "pts", 3).view(-1, 3), f32(nrm, "nrm", 3).view(-1, 3), f32(cells, "cells", 8).view(-1, 8)
    frames, maps = _shadow_inputs(frames, maps)
    if pts.shape != nrm.shape or cells.shape[0] != frames.shape[0]:
        raise ValueError("shadow_lookup: one normal per point and one frame per cell")
    vis = torch.empty((pts.shape[0], cells.shape[0]), dtype=torch.uint8, device=pts.device)
    _call("tir_shadow_lookup", _ptr(pts), _ptr(nrm), _ptr(cells), _ptr(frames), _ptr(maps), pts.shape[0], cells.shape[0], maps.shape[1],
          float(bias[0]), float(bias[1]), _ptr(vis), _stream())
    return vis


def light_gbuffer_shadowed(gbuf, view, cells, pts, frames, maps, bias, fresnel=0.04, occlusion=True, srgb=False):
    """tir_light_gbuffer_shadowed: light_gbuffer with pts [..., 3] (each row's surface point in the frames' coordinates): a cell
    lights a row only where shadow_lookup's rule says lit.  -> [..., 4] = {r, g, b, coverage}."""
    gbuf, view, cells = f32(gbuf, "gbuf", RASTER_ROW), f32(view, "view", 3), f32(cells, "cells", 8).view(-1, 8)
    pts = f32(pts, "pts", 3)
    frames, maps = _shadow_inputs(frames, maps)
    if gbuf.shape[:-1] != view.shape[:-1] or gbuf.shape[:-1] != pts.shape[:-1]:
        raise ValueError("light_gbuffer_shadowed: gbuf, view and pts take one row per pixel")
    if cells.shape[0] != frames.shape[0]:
        raise ValueError("light_gbuffer_shadowed: one frame per light cell")
    out = torch.empty(gbuf.shape[:-1] + (4,), dtype=torch.float32, device=gbuf.device)
    flags = (LIGHT_OCCLUSION if occlusion else 0) | (LIGHT_SRGB if srgb else 0)
    _call("tir_light_gbuffer_shadowed", _ptr(gbuf), _ptr(view), _ptr(cells), _ptr(pts), _ptr(frames), _ptr(maps),
          gbuf.numel() // RASTER_ROW, cells.shape[0], maps.shape[1], float(bias[0]), float(bias[1]), float(fresnel), flags, _ptr(out),
          _stream())
    return out


# ---- traced shadows of the exported asset: one any-hit ray per (point, light cell) pair (tensoir_amd/raster.py) ----
def _occl_words(M):
    return (int(M) + 63) // 64


def shadow_trace(pts, nrm, cells, verts, faces, grid=None, t0=0.0):
    """tir_shadow_trace: pts, nrm [M, 3] (surface points and their stored normals), cells [D, 8] (env_cells), verts [V, 3] f32 and
    faces [F, 3] i32 on one GPU; grid: face_grid(verts, faces) of THIS mesh (None builds the default one) -> occl [D, ceil(M / 64)]
    int64: bit m & 63 of word [d, m >> 6] is 1 iff pair (m, d) contributes (n.L > 1e-6, as light_gbuffer forms it) and the ray from
    pts[m] along cells[d]'s direction over [t0, +inf] meets the mesh by ray_mesh's rule (mode "any").  Every other bit is 0.
    The bits are identical for every grid over the same faces.  No read-back when a grid is handed in."""
    pts, nrm, cells = f32(pts, "pts", 3).view(-1, 3), f32(nrm, "nrm", 3).view(-1, 3), f32(cells, "cells", 8).view(-1, 8)
    verts, faces = _mesh_args(verts, faces)
    dev = verts.device
    if pts.shape != nrm.shape:
        raise ValueError("shadow_trace: one normal per point")
    if cells.shape[0] < 1:
        raise ValueError("shadow_trace: at least one light cell")
    if any(x.device != dev for x in (pts, nrm, cells)):
        raise ValueError("pts, nrm, cells: expected the device of verts")
    t0 = float(t0)
    if not (t0 >= 0.0 and math.isfinite(t0)):
        raise ValueError("shadow_trace: t0 is finite and >= 0")
    grid = _ray_grid(verts, faces, grid, "shadow_trace")
    M, D, V, F, P = pts.shape[0], cells.shape[0], verts.shape[0], faces.shape[0], grid["n_pairs"]
    occl = torch.empty((D, _occl_words(M)), dtype=torch.int64, device=dev)
    _call("tir_shadow_trace", _ptr(pts if M else None), _ptr(nrm if M else None), _ptr(cells), M, D, _ptr(verts if V else None), V,
          _ptr(faces if F else None), F, (C.c_float * 3)(*grid["cell"]), (C.c_float * 3)(*grid["origin"]), (C.c_int32 * 3)(*grid["dims"]),
          _ptr(grid["cursor"]), _ptr(grid["pairs"] if P else None), P, _ptr(grid["bounds"]), t0, _ptr(occl if M else None), _stream())
    return occl


def occlusion_bits(occl, M):
    """occl [D, ceil(M / 64)] int64 (shadow_trace) -> bool [M, D]: pair (m, d) is occluded.  Plain torch, for tests and diagnostics."""
    occl = torch.as_tensor(occl)
    M = int(M)
    if occl.dtype != torch.int64 or occl.dim() != 2 or occl.shape[1] != _occl_words(M):
        raise ValueError("occlusion_bits: occl is [D, ceil(M / 64)]")
    shifts = torch.arange(64, dtype=torch.int64, device=occl.device)
    bits = ((occl[:, :, None] >> shifts) & 1) != 0                        # (an arithmetic shift: the mask keeps the one bit)
    return bits.reshape(occl.shape[0], -1)[:, :M].t().contiguous()


def pack_occlusion(mask):
    """bool [M, D] -> occl [D, ceil(M / 64)] int64, the layout of shadow_trace (rows beyond M: 0).  Plain torch."""
    mask = torch.as_tensor(mask)
    if mask.dim() != 2:
        raise ValueError("pack_occlusion: mask is [M, D]")
    M, D = mask.shape
    W = _occl_words(M)
    b = torch.zeros((D, W * 64), dtype=torch.int64, device=mask.device)
    b[:, :M] = (mask != 0).t().to(torch.int64)
    shifts = torch.arange(64, dtype=torch.int64, device=mask.device)
    return (b.view(D, W, 64) << shifts).sum(-1).contiguous()              # (bit 63 wraps into the sign: the sum is exact mod 2^64)


def light_gbuffer_occluded(gbuf, view, cells, occl, fresnel=0.04, occlusion=True, srgb=False):
    """tir_light_gbuffer_occluded: light_gbuffer with occl [D, >= ceil(M / 64)] int64 (shadow_trace of the same rows and cells): a
    cell lights a row only where the pair's bit is 0.  -> [..., 4] = {r, g, b, coverage}."""
    gbuf, view, cells = f32(gbuf, "gbuf", RASTER_ROW), f32(view, "view", 3), f32(cells, "cells", 8).view(-1, 8)
    occl = _req(occl, torch.int64, "occl")
    if gbuf.shape[:-1] != view.shape[:-1]:
        raise ValueError("light_gbuffer_occluded: gbuf and view take one row per pixel")
    M, D = gbuf.numel() // RASTER_ROW, cells.shape[0]
    if D < 1:
        raise ValueError("light_gbuffer_occluded: at least one light cell")
    if occl.dim() != 2 or occl.shape[0] != D or occl.shape[1] < _occl_words(M) or occl.device != gbuf.device:
        raise ValueError("light_gbuffer_occluded: occl is [D, ceil(M / 64)] int64 on gbuf's device (shadow_trace)")
    out = torch.empty(gbuf.shape[:-1] + (4,), dtype=torch.float32, device=gbuf.device)
    flags = (LIGHT_OCCLUSION if occlusion else 0) | (LIGHT_SRGB if srgb else 0)
    _call("tir_light_gbuffer_occluded", _ptr(gbuf), _ptr(view), _ptr(cells), _ptr(occl if M else None), occl.shape[1], M, D,
          float(fresnel), flags, _ptr(out), _stream())
    return out


# ---- image metrics (tensoir_amd/metrics.py) -----------------------------------------------------------------------
SSIM_TILE = _K["TIR_SSIM_TILE"]                   # the side of the output tile one workgroup of tir_ssim computes
SSIM_MAX_TAPS = _K["TIR_SSIM_MAX_TAPS"]
IMAGE_ERROR_SHARE = _K["TIR_IMAGE_ERROR_SHARE"]   # pixels per workgroup of tir_image_error (at most 256 workgroups per image)


def _workspace(doubles, dev):
    if doubles < 0:
        check(int(doubles), "metrics workspace")
    return torch.empty((int(doubles),), dtype=torch.float64, device=dev)


def ssim(img0, img1, taps, c1, c2, return_map=False):
    """tir_ssim: img0, img1 [N, H, W, C] f32 on the device (1 <= C <= 4), taps: a float64 numpy vector of 1..SSIM_MAX_TAPS filter
    weights (host) -> mean [N] float64 on the device, and with return_map also the map [N, H - n + 1, W - n + 1, C] float64.  fp32
    products, double sums, a fixed-order mean (see the header); the host does not wait."""
    img0, img1 = f32(img0, "img0"), f32(img1, "img1")
    if img0.dim() != 4 or img0.shape != img1.shape or img0.device != img1.device:
        raise ValueError(f"ssim: two [N, H, W, C] images of one shape on one device, got {tuple(img0.shape)} and {tuple(img1.shape)}")
    taps = np.ascontiguousarray(taps, dtype=np.float64).reshape(-1)
    N, H, W, Cn = img0.shape
    n = taps.shape[0]
    ws = _workspace(lib().tir_ssim_workspace(N, H, W, Cn, n), img0.device)          # the library words a refusal of the shape
    mean = torch.empty((N,), dtype=torch.float64, device=img0.device)
    smap = torch.empty((N, H - n + 1, W - n + 1, Cn), dtype=torch.float64, device=img0.device) if return_map else None
    with torch.cuda.device(img0.device):
        _call("tir_ssim", _ptr(img0), _ptr(img1), N, H, W, Cn, C.c_void_p(taps.ctypes.data), n, float(c1), float(c2), _ptr(smap), _ptr(ws),
              _ptr(mean), _stream())
    return (mean, smap) if return_map else mean


def image_error(a, b, mask=None, angular=False):
    """tir_image_error: a, b [N, P, C] f32 on the device, mask None or [N, P] uint8 / bool -> [N, 3] float64 on the device:
    {pixels counted, sum of (a - b)^2 over them and their channels, sum of acos(clamp(a . b, -1, 1)) in degrees (C = 3 with
    angular, else 0)}.  Nothing is normalised; fixed-order sums; the host does not wait."""
    a, b = f32(a, "a"), f32(b, "b")
    if a.dim() != 3 or a.shape != b.shape or a.device != b.device:
        raise ValueError(f"image_error: two [N, P, C] images of one shape on one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    N, P, Cn = a.shape
    if mask is not None:
        mask = _req(mask.view(torch.uint8) if mask.dtype == torch.bool else mask, torch.uint8, "mask")
        if mask.shape != (N, P) or mask.device != a.device:
            raise ValueError("image_error: mask is [N, P] on the images' device")
    ws = _workspace(lib().tir_image_error_workspace(N, P), a.device)
    out = torch.zeros((N, 3), dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _call("tir_image_error", _ptr(a), _ptr(b), _ptr(mask), N, P, Cn, int(bool(angular)), _ptr(ws), _ptr(out), _stream())
    return out


# ---- total-variation regulariser (tensoir_amd/regularisers.py) ----------------------------------------------------
TV_MAX_PLANES = _K["TIR_TV_MAX_PLANES"]           # planes per launch
TV_SHARE = _K["TIR_TV_SHARE"]                     # floats of one plane per workgroup of tir_tv_bwd, and of tir_tv_fwd on a small plane
TV_FWD_GROUPS = _K["TIR_TV_FWD_GROUPS"]           # tir_tv_fwd gives a plane at most this many workgroups (larger shares beyond)


def is_channel_last(t):
    """A [1, C, H, W] float32 tensor stored as [H][W][C] in memory -- the layout the kernels gather from (field_model.channel_last
    makes one; a unit dimension's stride is free)."""
    if t.dim() != 4 or t.shape[0] != 1 or t.dtype != torch.float32:
        return False
    _, c, h, w = t.shape
    _, sc, sh, sw = t.stride()
    return (c == 1 or sc == 1) and (w == 1 or sw == c) and (h == 1 or sh == w * c)


def _on_device(t, dtype, name):
    """_req's checks without its .contiguous(): a channel-last plane is not contiguous in torch's default format, and a copy of it
    would be a plane-sized launch and allocation per call -- the planes are read in place."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise _lib.TensoirHipError(f"{name}: tensor must live on the GPU (got {t.device}); tensoir_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


class _TvCall:
    """The one place the TV entry points' arguments are validated and laid out: planes -> the host arrays of a call."""

    def __init__(self, planes, coefs, what):
        planes = list(planes)
        n = len(planes)
        if n > TV_MAX_PLANES or len(coefs) != n:
            raise ValueError(f"{what}: at most {TV_MAX_PLANES} planes and one coefficient per plane, got {n} and {len(coefs)}")
        for i, t in enumerate(planes):
            _on_device(t, torch.float32, f"{what}: plane {i}")
            if not is_channel_last(t) or t.shape[2] < 2 or t.shape[3] < 2 or t.device != planes[0].device:
                raise ValueError(f"{what}: plane {i} must be [1, C, H >= 2, W >= 2] in channel-last storage on one device, got "
                                 f"{tuple(t.shape)} with strides {tuple(t.stride())} on {t.device}")
        self.n, self.planes = n, planes
        self.device = planes[0].device if n else None
        self.ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in planes])
        self.C = (C.c_int32 * n)(*[t.shape[1] for t in planes])
        self.H = (C.c_int32 * n)(*[t.shape[2] for t in planes])
        self.W = (C.c_int32 * n)(*[t.shape[3] for t in planes])
        self.coef = (C.c_double * n)(*[float(c) for c in coefs])


def tv_forward(planes, coefs):
    """tir_tv_fwd: planes, a list of at most TV_MAX_PLANES float32 [1, C, H, W] device tensors in channel-last storage (H, W >= 2),
    coefs one host float per plane -> (loss, a 0-dim float32 = sum_p coefs[p] 2 (Sh_p / nh_p + Sw_p / nw_p), sums [n, 2] float64 =
    {Sh_p, Sw_p}), both on the device.  One launch; fp32 differences and squares, double sums in a fixed order (see the header);
    the host does not wait."""
    call = _TvCall(planes, coefs, "tv_forward")
    if call.n == 0:
        raise ValueError("tv_forward: no planes")
    ws = _workspace(lib().tir_tv_workspace(call.n, call.C, call.H, call.W), call.device)
    sums = torch.empty((call.n, 2), dtype=torch.float64, device=call.device)
    loss = torch.empty((), dtype=torch.float32, device=call.device)
    with torch.cuda.device(call.device):
        _call("tir_tv_fwd", call.ptrs, call.C, call.H, call.W, call.coef, call.n, _ptr(ws), _ptr(sums), _ptr(loss), _stream())
    return loss, sums


def tv_backward(planes, coefs, g, needs=None, out=None):
    """tir_tv_bwd: the gradient of tv_forward's loss times the DEVICE scalar g (float32, one element; never read on the host) for
    every plane p with needs[p] (default: all) -> a list with a channel-last [1, C, H, W] tensor per wanted plane and None for the
    others.  out: optional list of channel-last tensors to write into (None entries are skipped like needs[p] = False).  One
    launch; every element of a wanted gradient is written, nothing else is touched."""
    call = _TvCall(planes, coefs, "tv_backward")
    g = _req(g, torch.float32, "tv_backward: g")
    if g.numel() != 1 or (call.n and g.device != call.device):
        raise ValueError(f"tv_backward: g is one float32 on the planes' device, got {tuple(g.shape)} on {g.device}")
    if out is None:
        needs = [True] * call.n if needs is None else list(needs)
        if len(needs) != call.n:
            raise ValueError("tv_backward: one flag per plane")
        out = [torch.empty((1, t.shape[2], t.shape[3], t.shape[1]), dtype=torch.float32, device=t.device).permute(0, 3, 1, 2)
               if want else None for t, want in zip(call.planes, needs)]
    else:
        out = list(out)
        if len(out) != call.n:
            raise ValueError("tv_backward: one output (or None) per plane")
        for i, (o, t) in enumerate(zip(out, call.planes)):
            if o is not None and (not torch.is_tensor(o) or o.shape != t.shape or o.device != t.device or not is_channel_last(o)):
                raise ValueError(f"tv_backward: out[{i}] must be a channel-last float32 tensor of plane {i}'s shape and device")
    if call.n == 0 or all(o is None for o in out):
        return out
    grads = (C.c_void_p * call.n)(*[None if o is None else o.data_ptr() for o in out])
    with torch.cuda.device(call.device):
        _call("tir_tv_bwd", call.ptrs, call.C, call.H, call.W, call.coef, call.n, _ptr(g), grads, _stream())
    return out


# ---- guided a-trous denoiser (tensoir_amd/denoise.py) -------------------------------------------------------------
DENOISE_GUIDE = _K["TIR_DENOISE_GUIDE"]           # floats of a guide row {pos.xyz, valid, n.xyz, roughness, albedo.rgb, 0}
ATROUS_MAX_K = _K["TIR_ATROUS_MAX_K"]             # colour floats per pixel of one tir_atrous_level launch (eight maps)


def denoise_guide(maps, rays, guide, row0, acc_thres=0.5):
    """tir_denoise_guide: maps [B, 20] (the primary pass's map rows) and rays [B, 6] -> rows [row0, row0 + B) of guide [N, 12]
    (or [H, W, 12]), written in place: {o + depth d, acc > acc_thres, the normalised normal, roughness, albedo, 0}.  One launch;
    the host does not wait.  Returns guide."""
    maps, rays = f32(maps, "maps", MAP_STRIDE), f32(rays, "rays", 6)
    _req(guide, torch.float32, "guide", DENOISE_GUIDE)
    B, row0 = maps.shape[0], int(row0)
    if maps.dim() != 2 or rays.dim() != 2 or rays.shape[0] != B or not guide.is_contiguous():
        raise ValueError(f"denoise_guide: maps [B, 20], rays [B, 6] and a contiguous guide, got {tuple(maps.shape)}, {tuple(rays.shape)}")
    if row0 < 0 or row0 + B > guide.numel() // DENOISE_GUIDE or maps.device != guide.device or rays.device != guide.device:
        raise ValueError(f"denoise_guide: rows [{row0}, {row0 + B}) must lie in a guide of {guide.numel() // DENOISE_GUIDE} rows "
                         "on the device of maps and rays")
    with torch.cuda.device(guide.device):
        _call("tir_denoise_guide", _ptr(maps), _ptr(rays), B, float(acc_thres), _ptr(guide), row0, _stream())
    return guide


def atrous_level(color_in, color_out, guide, H, W, step, inv_sn, inv_sp, inv_sa2, inv_sr2, inv_sc2=0.0):
    """tir_atrous_level: one level of the guided a-trous filter, out of place.  color_in, color_out [H * W, K] f32 (any shape of
    H * W * K contiguous floats; K = 3 n_maps, 3..ATROUS_MAX_K), guide [H * W, 12] -> color_out.  step >= 1: the distance between
    taps; inv_*: 1 / sigma_n, 1 / sigma_p, 1 / sigma_a^2, 1 / sigma_r^2, 1 / sigma_c^2 (0: no colour term).  fp32, a fixed
    order of taps (see the header); the host does not wait."""
    color_in, guide = f32(color_in, "color_in"), f32(guide, "guide", DENOISE_GUIDE)
    _req(color_out, torch.float32, "color_out")
    H, W = int(H), int(W)
    if H < 1 or W < 1 or color_in.numel() % (H * W) or not color_out.is_contiguous():
        raise ValueError(f"atrous_level: color_in holds {color_in.numel()} floats, no multiple of {H} x {W}; color_out is contiguous")
    K = color_in.numel() // (H * W)
    if color_out.numel() != color_in.numel() or guide.numel() != H * W * DENOISE_GUIDE:
        raise ValueError(f"atrous_level: color_out takes {H * W * K} floats and guide {H * W} rows, got {color_out.numel()} and "
                         f"{guide.numel() // DENOISE_GUIDE}")
    if color_out.device != color_in.device or guide.device != color_in.device:
        raise ValueError("atrous_level: color_in, color_out and guide live on one device")
    with torch.cuda.device(color_in.device):
        _call("tir_atrous_level", _ptr(color_in), _ptr(color_out), _ptr(guide), H, W, K, int(step), float(inv_sn), float(inv_sp),
              float(inv_sa2), float(inv_sr2), float(inv_sc2), _stream())
    return color_out


# ---- material editing (tensoir_amd/materials.py) ---------------------------------------------------------------------
MATERIAL_MAX_EDITS = _K["TIR_MATERIAL_MAX_EDITS"]
MATERIAL_EDIT_FLOATS = _K["TIR_MATERIAL_EDIT_FLOATS"]       # floats of one edit record (layout: include/tensoir_hip.h)
MATERIAL_MAX_PALETTE = _K["TIR_MATERIAL_MAX_PALETTE"]
KMEANS_ROWS = _K["TIR_KMEANS_ROWS"]                         # rows per workgroup of tir_kmeans_assign


def _rows(t, name, width):
    """An fp32 device matrix whose rows are `width` contiguous floats at any row stride (a column view of a wider row is taken
    as it is, never copied) -> (tensor, row stride in floats)."""
    _req(t, torch.float32, name)
    if width == 1 and t.dim() == 1:
        t = t.unsqueeze(1)
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f"{name}: expected [M, {width}], got {tuple(t.shape)}")
    if (width > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < width):
        t = t.contiguous()
    return t, (int(t.stride(0)) if t.shape[0] > 1 else width)


def _edit_list(records, centroids):
    records = f32(records, "records", MATERIAL_EDIT_FLOATS).view(-1, MATERIAL_EDIT_FLOATS)
    k = 0
    if centroids is not None:
        centroids = f32(centroids, "centroids", 4).view(-1, 4)
        k = centroids.shape[0]
    return records, records.shape[0], centroids, k


def material_edit(records, centroids, rough_weight, points, albedo, rough, fresnel, m_dev=None):
    """tir_material_edit: the edit list `records` [n, 32] (palette `centroids` [k, 4] or None, roughness weight) on M rows of
    points [M, 3], albedo [M, 3], rough [M] or [M, 1], fresnel [M, 3] -- column views of wider rows are read in place -- ->
    dict(albedo, roughness, fresnel, base, metal), new dense tensors.  m_dev (int32 device scalar): only the first min(M, m_dev)
    rows exist; the rows beyond are not written (they hold what torch.empty left)."""
    records, n, centroids, k = _edit_list(records, centroids)
    (points, ps), (albedo, as_), (rough, rs), (fresnel, fs) = (_rows(points, "points", 3), _rows(albedo, "albedo", 3),
                                                              _rows(rough, "roughness", 1), _rows(fresnel, "fresnel", 3))
    M, dev = albedo.shape[0], albedo.device
    if not (points.shape[0] == rough.shape[0] == fresnel.shape[0] == M):
        raise ValueError(f"material_edit: {points.shape[0]} points, {M} albedo, {rough.shape[0]} roughness and {fresnel.shape[0]} "
                         "fresnel rows")
    v3 = lambda: torch.empty((M, 3), dtype=torch.float32, device=dev)
    v1 = lambda: torch.empty((M,), dtype=torch.float32, device=dev)
    out = {"albedo": v3(), "roughness": v1(), "fresnel": v3(), "base": v3(), "metal": v1()}
    with torch.cuda.device(dev):
        _call("tir_material_edit", _ptr(records if n else None), n, _ptr(centroids), k, float(rough_weight), _ptr(points), ps,
              _ptr(albedo), as_, _ptr(rough), rs, _ptr(fresnel), fs, _ptr(out["albedo"]), _ptr(out["roughness"]), _ptr(out["fresnel"]),
              _ptr(out["base"]), _ptr(out["metal"]), M, _ptr(m_dev), _stream())
    return out


def material_edit_maps(records, centroids, rough_weight, maps, rays, acc_thres=0.5):
    """tir_material_edit_maps: the edit list on the rows of a chunk's primary maps [B, 20] with acc > acc_thres, IN PLACE on their
    albedo, roughness and Fresnel columns; the position is surface_compact's surf.  maps must be contiguous (it is written)."""
    records, n, centroids, k = _edit_list(records, centroids)
    _req(maps, torch.float32, "maps", MAP_STRIDE)
    rays = f32(rays, "rays", 6)
    if maps.dim() != 2 or not maps.is_contiguous() or rays.dim() != 2 or rays.shape[0] != maps.shape[0] or rays.device != maps.device:
        raise ValueError(f"material_edit_maps: a contiguous maps [B, 20] and rays [B, 6] on its device, got {tuple(maps.shape)}, "
                         f"{tuple(rays.shape)}")
    with torch.cuda.device(maps.device):
        _call("tir_material_edit_maps", _ptr(records if n else None), n, _ptr(centroids), k, float(rough_weight), _ptr(maps), _ptr(rays),
              maps.shape[0], float(acc_thres), _stream())
    return maps


def atlas_metal(orm, cols, T, n_faces, metal):
    """tir_atlas_metal: the B channel of atlas_pack's orm image [size, size, 4] uint8 = round(255 metal) on the owned texels, in
    place (metal [N]: cell-major, as atlas_texels orders the texels)."""
    if orm.dtype != torch.uint8 or not orm.is_cuda or orm.dim() != 3 or orm.shape[0] != orm.shape[1] or orm.shape[2] != 4 \
            or not orm.is_contiguous():
        raise ValueError("atlas_metal: orm is a contiguous [size, size, 4] uint8 image on the GPU")
    metal = f32(metal, "metal").view(-1)
    N = ((int(n_faces) + 1) // 2) * int(T) * int(T)
    if metal.shape[0] != N:
        raise ValueError(f"atlas_metal: metal takes {N} rows (ceil(F / 2) * T * T), got {metal.shape[0]}")
    with torch.cuda.device(orm.device):
        _call("tir_atlas_metal", _ptr(orm), int(orm.shape[0]), int(cols), int(T), int(n_faces), _ptr(metal if N else None), _stream())
    return orm


def kmeans_seed(albedo, rough, k, rough_weight=1.0):
    """k farthest-point seeds from row 0 (tir_kmeans_seed, k launches of one step) -> centroids [k, 4]."""
    albedo, rough = f32(albedo, "albedo", 3).view(-1, 3), f32(rough, "roughness").view(-1)
    N, dev = albedo.shape[0], albedo.device
    centroids = torch.zeros((int(k), 4), dtype=torch.float32, device=dev)
    mind = torch.empty((max(N, 1),), dtype=torch.float32, device=dev)
    best = torch.zeros((1,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        for have in range(int(k)):
            _call("tir_kmeans_seed", _ptr(albedo), _ptr(rough), N, float(rough_weight), _ptr(centroids), int(k), have, _ptr(mind),
                  _ptr(best), _stream())
    return centroids


def kmeans_workspace(N, k, dev):
    """The buffers a Lloyd pass leaves its partials in: (part_sums [G, k, 5] f64, part_counts [G, k] i32, part_changed [G] i32)."""
    G = int(lib().tir_kmeans_groups(int(N)))
    if G < 0:
        check(G, "tir_kmeans_groups")
    return (torch.empty((G, k, 5), dtype=torch.float64, device=dev), torch.empty((G, k), dtype=torch.int32, device=dev),
            torch.empty((G,), dtype=torch.int32, device=dev))


def kmeans_assign(albedo, rough, centroids, labels, workspace, first, rough_weight=1.0):
    """tir_kmeans_assign: labels [N] int32 (in place) = the nearest centroid of every row, the lowest index among equals, and the
    per-workgroup partial sums / counts / changed-label counts in `workspace` (kmeans_workspace)."""
    albedo, rough = f32(albedo, "albedo", 3).view(-1, 3), f32(rough, "roughness").view(-1)
    centroids = f32(centroids, "centroids", 4)
    i32(labels, "labels")
    sums, counts, changed = workspace
    if not labels.is_contiguous() or labels.shape[0] != albedo.shape[0]:
        raise ValueError("kmeans_assign: labels is a contiguous [N] int32 tensor")
    with torch.cuda.device(albedo.device):
        _call("tir_kmeans_assign", _ptr(albedo), _ptr(rough), albedo.shape[0], float(rough_weight), _ptr(centroids), centroids.shape[0],
              int(bool(first)), _ptr(labels), _ptr(sums), _ptr(counts), _ptr(changed), sums.shape[0], _stream())
    return labels


def kmeans_update(workspace, centroids, counts, inertia, changed):
    """tir_kmeans_update: the partials of one assignment, added in workgroup order -> centroids [k, 4] (in place; an empty cluster
    keeps its centroid), counts [k] int64, inertia [1] float64, changed [1] int32."""
    sums, pc, pch = workspace
    if not centroids.is_contiguous() or centroids.dtype != torch.float32 or centroids.shape[0] != sums.shape[1]:
        raise ValueError("kmeans_update: centroids is the contiguous fp32 [k, 4] tensor the assignment read")
    with torch.cuda.device(centroids.device):
        _call("tir_kmeans_update", _ptr(sums), _ptr(pc), _ptr(pch), sums.shape[0], _ptr(centroids), centroids.shape[0], _ptr(counts),
              _ptr(inertia), _ptr(changed), _stream())
