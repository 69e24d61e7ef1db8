"""Packed MXQ weights (format v1, csrc/mxq_format.h) and the ops on them.

Every function here is a thin host wrapper: validate like the reference's launchers
should have (SURVEY.md 8b "Errors"), allocate outputs with torch, pass raw device pointers
and torch's current HIP stream to libmxq_hip.so.  No arithmetic happens in Python and
there is no CPU path: tensors must live on a ROCm device.

Reference semantics implemented by the kernels:
  quantize_pack  MXQGPT.fasterquant       mxq_quant/lib/mxqgpt.py:387-448
  unpack         Quantizer.quantize codes mxq_quant/lib/quantizer.py:14-16
  dequant        Quantizer.dequantize     mxq_quant/lib/quantizer.py:19-20 (+ fp16 cast, mxqgpt.py:448)
  linear         nn.Linear on that weight mxq_quant/main.py:85 / gemv_mxq_cuda.cu:39-208
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _lib

_TORCH2CODE = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}

PARAM_KEYS = ("codes2", "sc2", "zero2", "qs2", "qz2", "codes4", "sc4", "zero4", "qs4", "qz4")


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


class _NoCtx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NOCTX = _NoCtx()


def _on_device(device: torch.device):
    """Context that makes `device` current for a launch -- nothing at all when it already is (the usual case: one process
    per GPU; torch.cuda.device() costs ~4 us of host time per call, a third of a small-token Linear's)."""
    idx = device.index
    return _NOCTX if idx is None or idx == torch.cuda.current_device() else torch.cuda.device(device)


class _Workspace:
    """A cached GEMM workspace (``buf``) and what it owns.

    ``capture_id``: the capture sequence that created it, None for an eager workspace.  ``head_ready``: its head has been
    zeroed -- eagerly, or by a memset recorded into its graph.

    A stream-K wait that expires (include/mxq_hip.h) writes the affected tile as NaN and flags the workspace.  The flag must
    reach the CALLER without anybody polling: every eager workspace owns 4 ints of pinned host memory (``mailbox``, a numpy
    view of ``box``) whose address sits in its head; the kernel stores its status there with system-scope stores, and every
    later hand-out of that workspace -- i.e. the next packing.linear / QuantLinear.forward call on it -- reads the mailbox
    (plain host memory, no synchronisation) and raises.  A starved launch therefore cannot feed NaN activations into a model
    for more than the launches already queued behind it.  MXQ_CHECK_WORKSPACE=1 checks synchronously after EVERY call
    instead (debugging).  (Capture workspaces have none: pinning host memory is not a capturable operation, and a captured
    graph's launches are replayed without passing through here -- they are watched by workspace_status() alone.)"""
    __slots__ = ("key", "dev", "buf", "capture_id", "box", "mailbox", "head_ready")

    def __init__(self, key: tuple, buf: torch.Tensor, capture_id: Optional[int]):
        self.key, self.dev, self.buf, self.capture_id = key, key[0], buf, capture_id
        self.box = torch.zeros(4, dtype=torch.int32).pin_memory() if capture_id is None else None
        self.mailbox = self.box.numpy() if self.box is not None else None
        self.head_ready = False

    def reset(self) -> None:
        """Clear the mailbox, zero the head and write the mailbox's address into it (stream-ordered; under capture the device
        operations are recorded into the graph)."""
        self.buf[:_lib.WS_HEAD_BYTES].zero_()
        if self.box is not None:
            self.mailbox[:] = 0
            self.buf[_lib.WS_MAILBOX_OFFSET:_lib.WS_MAILBOX_OFFSET + 8].view(torch.int64).fill_(self.box.data_ptr())
        self.head_ready = True


_WORKSPACES: Dict[tuple, _Workspace] = {}   # (device, stream) or (device, "capture", capture id, bytes) -> workspace
_CHECK_EVERY_CALL = __import__("os").environ.get("MXQ_CHECK_WORKSPACE", "") not in ("", "0")
# A capture workspace lives in its graph's private memory pool; this cache holds a reference so that the memory cannot be
# handed to a later capture that shares the pool while the first graph still replays on it.  The price is that
# the bytes stay pinned after their graph is gone, so the cache is bounded -- generously: 256 graphs of <= 67 MB.
_CAPTURES: deque = deque()      # capture workspaces in order of creation
_MAX_CAPTURE_WS = 256


def _capture_id(stream_handle: int):
    """(capturing?, id of the capture sequence) of a stream, asked through libmxq_hip.so's own HIP runtime
    (include/mxq_hip.h: mxq_stream_capture_id -- never a second runtime opened by name)."""
    import ctypes
    active, cid = ctypes.c_int(0), ctypes.c_ulonglong(0)
    _lib.check(_lib.load().mxq_stream_capture_id(ctypes.c_void_p(stream_handle), ctypes.byref(active), ctypes.byref(cid)),
               "mxq_stream_capture_id")
    return bool(active.value), int(cid.value)


def gemm_workspace(device: torch.device, counters: bool = True, stream: Optional[int] = None,
                   need: Optional[int] = None) -> Optional[torch.Tensor]:
    """Scratch buffer of the stream-K prefill GEMM and of the mid-M kernel's partial tiles (include/mxq_hip.h:
    mxq_linear_f16_ws).  Its counter head must be zero when a stream-K launch starts; the kernels leave it zeroed.

    Eager launches: one buffer of the maximum size per (device, stream), created and zeroed on first use -- launches on
    one stream run in order and may share it, launches on different streams may not.

    Captured launches: buffers per CAPTURED GRAPH (keyed by the capture sequence's id), so two graphs replayed at the same
    time on two streams never share partial sums or counters.  ``need`` (bytes this launch can use,
    mxq_linear_workspace_need; None = the maximum) sizes them: a graph whose launches never leave the skinny kernel gets
    none at all (``need`` 0 returns None), one that stays within the small-tile builds a 34-MB buffer instead of 67 MB
    (two size classes per graph at most).  A buffer born under capture is never zeroed for real until a replay runs: its
    first counters hand-out records ONE memset of the counter head into the graph.

    ``counters=False``: the caller's kernel uses the buffer beyond the head only (the mid-M kernel's partial tiles):
    no memset is recorded for it."""
    if need is not None and need <= 0:
        return None
    dev_index = device.index if device.index is not None else torch.cuda.current_device()
    if stream is None:                      # (callers on the hot path pass the handle they already hold)
        stream = torch.cuda.current_stream(device).cuda_stream
    lib = _lib.load()
    full = lib.mxq_gemm_workspace_bytes()
    # (torch's own query looks at the CURRENT device's stream; only when it says "capturing" -- or the device is another
    #  one -- is the stream itself asked, through the library)
    capturing, cid = False, 0
    if dev_index != torch.cuda.current_device() or torch.cuda.is_current_stream_capturing():
        capturing, cid = _capture_id(stream)
    if capturing:
        nbytes = full if need is None or 2 * need > full else (full + _lib.WS_HEAD_BYTES) // 2     # two size classes
        nbytes = max(nbytes, need or 0)
        key = (dev_index, "capture", cid, nbytes)
        ws = _WORKSPACES.get(key)
        if ws is None:                      # a bigger buffer of the same graph serves a smaller need
            ws = _WORKSPACES.get((dev_index, "capture", cid, full))
    else:
        nbytes, key = full, (dev_index, stream)
        ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _WORKSPACES[key] = _Workspace(key, torch.empty(nbytes, dtype=torch.uint8, device=device),
                                           cid if capturing else None)
        if capturing:                       # zeroed when a counters hand-out records the memset (below)
            _CAPTURES.append(ws)
            if len(_CAPTURES) > _MAX_CAPTURE_WS:
                del _WORKSPACES[_CAPTURES.popleft().key]
        else:
            ws.reset()
    elif ws.mailbox is not None and ws.mailbox[0] != 0:   # a launch that ran on this workspace since the last hand-out gave up a wait
        _raise_expired(ws)
    if capturing and counters and not ws.head_ready:
        ws.reset()                          # recorded once per graph and buffer
    return ws.buf


def _cached_by_device(device: Optional[torch.device]) -> Dict[int, list]:
    """The cached workspaces by device index: all devices', or ``device``'s alone."""
    only = None if device is None else (device.index if device.index is not None else torch.cuda.current_device())
    by_dev: Dict[int, list] = {}
    for ws in _WORKSPACES.values():
        if only is None or ws.dev == only:
            by_dev.setdefault(ws.dev, []).append(ws)
    return by_dev


def _reset_synchronised(dev_index: int, workspaces) -> None:
    """Reset ``workspaces`` (all on device ``dev_index``) after the device's queued work, and wait for the resets."""
    with torch.cuda.device(dev_index):
        torch.cuda.synchronize(dev_index)
        for ws in workspaces:
            ws.reset()
        torch.cuda.synchronize(dev_index)


def _raise_expired(ws: _Workspace):
    """The mailbox of ``ws`` is set: report, make the workspace usable again (synchronises), raise."""
    st = [int(v) for v in ws.mailbox]
    _reset_synchronised(ws.dev, [ws])
    raise RuntimeError(f"stream-K wait expired on workspace {ws.key}: [code, tail tile, workgroup, count seen] = {st}; the affected "
                       "output tiles of that launch are NaN (results computed since then on this stream are suspect); the "
                       "workspace has been reset")


_HOIST: Dict[tuple, torch.Tensor] = {}
HOIST_MIN_TOKENS = 4096     # mxq_hoist_min_tokens(): "auto" hoists the dequant out of the token loop from this many tokens on


def hoist_scratch(device: torch.device, nbytes: int) -> torch.Tensor:
    """Transient fp16-weight scratch of the hoisted-dequant mode (include/mxq_hip.h: mxq_linear_f16_hoisted), one per
    (device, stream), grown on demand.  Nothing is cached in it between calls: every call rewrites it first."""
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    buf = _HOIST.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _HOIST[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return buf


def _layout_code(p) -> int:
    if isinstance(p, PackedMXQ):
        return 3 if p.compact else 0
    return LAYOUTS[p.layout]


def linear_hoisted(x: torch.Tensor, p, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Quantised Linear with the dequant hoisted out of the token loop (dequant kernel once into a scratch buffer,
    then the MFMA kernel on fp16 tiles): bit-identical to the fused GEMM, faster from HOIST_MIN_TOKENS (4096) tokens per
    launch (profiles/r03_dense256.txt)."""
    _need_gpu(x, p.qweight)
    if x.dtype != torch.float16 or x.shape[-1] != p.K:
        raise ValueError("activations must be fp16 [..., in_features]")
    x2 = x.reshape(-1, p.K).contiguous()
    M = x2.shape[0]
    if out is None:
        out = torch.empty((M, p.N), dtype=torch.float16, device=x.device)
    if M == 0:
        return out.reshape(*x.shape[:-1], p.N)
    lib = _lib.load()
    scratch = hoist_scratch(x2.device, lib.mxq_hoist_scratch_bytes(p.N, p.K))
    with _on_device(x.device):
        _lib.check(lib.mxq_linear_f16_hoisted(x2.data_ptr(), p.qweight.data_ptr(), p.rowmeta.data_ptr(), out.data_ptr(),
                                              M, p.N, p.K, _layout_code(p), scratch.data_ptr(), scratch.numel(),
                                              _stream(x2)), "mxq_linear_f16_hoisted")
    return out.reshape(*x.shape[:-1], p.N)


def workspace_status(device: Optional[torch.device] = None, reset: bool = True) -> None:
    """Raise RuntimeError if a stream-K wait gave up on any cached workspace (all devices, or one) since the last check
    (include/mxq_hip.h: mxq_workspace_status -- the affected tiles were written as NaN).  Synchronises the workspace's
    stream; call it wherever the caller synchronises anyway (end of a prefill, a test, a bench's timed region).
    ``reset``: re-zero the counter head of a flagged workspace so that it can be used again."""
    import ctypes
    lib = _lib.load()
    bad = []
    st = (ctypes.c_int * 4)()
    for dev_index, workspaces in _cached_by_device(device).items():
        flagged = []
        with torch.cuda.device(dev_index):
            torch.cuda.synchronize(dev_index)          # (capture workspaces have no eager stream of their own)
            for ws in workspaces:
                if not ws.head_ready:       # a capture workspace handed out with counters=False only: no stream-K launch
                    continue                # has seen it and its head was never written -- there is no status in it
                _lib.check(lib.mxq_workspace_status(ws.buf.data_ptr(), ws.buf.numel(), ctypes.cast(st, ctypes.c_void_p), None),
                           "mxq_workspace_status")
                if st[0] != 0:
                    bad.append((ws.key, list(st)))
                    flagged.append(ws)
        if reset and flagged:
            _reset_synchronised(dev_index, flagged)
    if bad:
        raise RuntimeError("stream-K wait expired (workspace key, [code, tail tile, workgroup, count seen]): "
                           f"{bad}; the affected output tiles are NaN" + ("; counter heads re-zeroed" if reset else ""))


def reset_gemm_workspace(device: Optional[torch.device] = None):
    """Re-zero the counter heads of the cached stream-K workspaces (all devices, or one).  Needed only after a
    GEMM launch was aborted mid-kernel (device reset, killed process sharing the buffer): the kernels themselves
    always leave the counters zeroed.  Synchronises the device(s) involved."""
    for dev_index, workspaces in _cached_by_device(device).items():
        _reset_synchronised(dev_index, workspaces)


def _need_gpu(*ts: torch.Tensor):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("mxq_amd ops run on the GPU only (no CPU fallback): got a CPU tensor")


def check_shape(N: int, K: int):
    if N <= 0 or K <= 0 or N % 16 != 0 or K % 64 != 0:
        raise ValueError(f"MXQ layout needs out_features % 16 == 0 and in_features % 64 == 0, got [{N}, {K}]")


def qweight_bytes(N: int, K: int) -> int:
    check_shape(N, K)
    return (N // 16) * (K // 64) * 576


@dataclass
class PackedMXQ:
    """qweight: int32 [N/16 * K/64 * 144] (576-B blocks, exact metadata) or [N/16 * K/64 * 120] (480-B blocks,
    ``compact``: fp16 zero-points, csrc/mxq_format.h MXQ_LAYOUT_MIXEDC); rowmeta: float32 [N, 4]."""
    qweight: torch.Tensor
    rowmeta: torch.Tensor
    N: int
    K: int
    compact: bool = False

    @property
    def device(self):
        return self.qweight.device

    def nbytes(self) -> int:
        return self.qweight.numel() * 4 + self.rowmeta.numel() * 4

    def bits_per_weight(self) -> float:
        return 8.0 * self.nbytes() / (self.N * self.K)


def concat_packed(ps):
    """Stack packed weights along the output dimension (e.g. q | k | v, or gate | up): format v1 is
    row-block-major, so this is a plain concatenation of the block arrays and of the row metadata, and one
    launch then computes all the stacked Linears of a shared input.  PackedUniform weights of one layout and one
    in_features stack the same way (the same [N/16][K/64] block grid)."""
    ps = list(ps)
    if ps and all(isinstance(p, PackedUniform) for p in ps):
        if any(p.K != ps[0].K or p.layout != ps[0].layout for p in ps):
            raise ValueError("concat_packed needs packed weights with the same in_features and layout")
        return PackedUniform(torch.cat([p.qweight for p in ps]), torch.cat([p.rowmeta for p in ps]),
                             sum(p.N for p in ps), ps[0].K, ps[0].layout)
    if any(not isinstance(p, PackedMXQ) for p in ps):
        raise ValueError("concat_packed needs packed weights of one kind: all PackedMXQ, or PackedUniform of one layout")
    if not ps or any(p.K != ps[0].K or p.compact != ps[0].compact for p in ps):
        raise ValueError("concat_packed needs packed weights with the same in_features and metadata mode")
    return PackedMXQ(torch.cat([p.qweight for p in ps]), torch.cat([p.rowmeta for p in ps]),
                     sum(p.N for p in ps), ps[0].K, ps[0].compact)


def compact(p: PackedMXQ) -> PackedMXQ:
    """Exact -> compact metadata (format "v2": the 2-bit zero-points as fp16; 3.75 instead of 4.5 bit/weight).  The
    integer codes, scale codes and (qs, qz) are unchanged, so ``unpack`` stays bit-exact on them; the dequantised
    weight moves by at most the fp16 rounding of a zero-point times its scale, the GEMM result by ~4e-4 relative
    (inside the 1e-3 budget: tests).  ``rowmeta`` is shared with ``p``."""
    if p.compact:
        return p
    _need_gpu(p.qweight)
    lib = _lib.load()
    nbytes = lib.mxq_qweight_bytes_layout(p.N, p.K, 3)
    q = torch.empty(nbytes // 4, dtype=torch.int32, device=p.device)
    with _on_device(p.device):
        _lib.check(lib.mxq_compact(p.qweight.data_ptr(), q.data_ptr(), p.N, p.K, _stream(q)), "mxq_compact")
    return PackedMXQ(q, p.rowmeta, p.N, p.K, True)


def _alloc(N: int, K: int, device) -> PackedMXQ:
    lib = _lib.load()
    nbytes = lib.mxq_qweight_bytes(N, K)
    assert nbytes == qweight_bytes(N, K)
    return PackedMXQ(torch.empty(nbytes // 4, dtype=torch.int32, device=device),
                     torch.empty((N, 4), dtype=torch.float32, device=device), N, K)


def quantize_pack(W: torch.Tensor, dead: Optional[torch.Tensor] = None, compact_meta: bool = False) -> PackedMXQ:
    """MXQ-quantise W [N, K] (fp16 / bf16 / fp32) on device and return the packed form (``compact_meta``: in the
    compact metadata mode, see ``compact``)."""
    _need_gpu(W, dead)
    if W.dim() != 2:
        raise ValueError("weight must be 2-D [out_features, in_features]")
    if W.dtype not in _TORCH2CODE:
        raise ValueError(f"unsupported weight dtype {W.dtype}")
    N, K = W.shape
    check_shape(N, K)
    W = W.contiguous()
    dead_p = None
    if dead is not None:
        if dead.numel() != K:
            raise ValueError("dead-column mask must have in_features entries")
        dead = dead.to(device=W.device, dtype=torch.uint8).contiguous()
        dead_p = dead.data_ptr()
    lib = _lib.load()
    p = _alloc(N, K, W.device)
    with _on_device(W.device):
        _lib.check(lib.mxq_quantize_pack(W.data_ptr(), _TORCH2CODE[W.dtype], dead_p, p.qweight.data_ptr(),
                                         p.rowmeta.data_ptr(), N, K, _stream(W)), "mxq_quantize_pack")
    return compact(p) if compact_meta else p


def _param_shapes(N: int, K: int) -> Dict[str, tuple]:
    G = 3 * K // 64
    return dict(codes2=((N, 3 * K // 4), torch.uint8), sc2=((N, G), torch.uint8), zero2=((N, G), torch.float32),
                qs2=((N // 16, G), torch.float32), qz2=((N // 16, G), torch.float32),
                codes4=((N, K // 4), torch.uint8), sc4=((N,), torch.uint8), zero4=((N,), torch.float32),
                qs4=((N // 16,), torch.float32), qz4=((N // 16,), torch.float32))


def pack_codes(params: Dict[str, torch.Tensor], N: int, K: int) -> PackedMXQ:
    """Pack integer codes + parameters (the output of Quantizer.quantize / find_params)."""
    check_shape(N, K)
    shapes = _param_shapes(N, K)
    ts = []
    for k in PARAM_KEYS:
        t = params[k]
        _need_gpu(t)
        shape, dt = shapes[k]
        if tuple(t.shape) != shape or t.dtype != dt:
            raise ValueError(f"{k}: expected {shape} {dt}, got {tuple(t.shape)} {t.dtype}")
        ts.append(t.contiguous())
    lib = _lib.load()
    p = _alloc(N, K, ts[0].device)
    with _on_device(p.device):
        _lib.check(lib.mxq_pack_codes(*[t.data_ptr() for t in ts], p.qweight.data_ptr(), p.rowmeta.data_ptr(), N, K,
                                      _stream(p.qweight)), "mxq_pack_codes")
    return p


def unpack(p: PackedMXQ) -> Dict[str, torch.Tensor]:
    """Integer unpack: codes and parameters exactly as packed."""
    _need_gpu(p.qweight)
    out = {k: torch.empty(shape, dtype=dt, device=p.device) for k, (shape, dt) in _param_shapes(p.N, p.K).items()}
    lib = _lib.load()
    fn = lib.mxq_unpack_compact if p.compact else lib.mxq_unpack
    with _on_device(p.device):
        _lib.check(fn(p.qweight.data_ptr(), p.rowmeta.data_ptr(), *[out[k].data_ptr() for k in PARAM_KEYS],
                      p.N, p.K, _stream(p.qweight)), "mxq_unpack")
    return out


def dequant(p) -> torch.Tensor:
    """Dense fp16 [N, K] fake-quant weight (bit-identical to the reference's write-back); a PackedUniform: ``dequant_uniform``."""
    if isinstance(p, PackedUniform):
        return dequant_uniform(p)
    _need_gpu(p.qweight)
    out = torch.empty((p.N, p.K), dtype=torch.float16, device=p.device)
    lib = _lib.load()
    fn = lib.mxq_dequant_f16_compact if p.compact else lib.mxq_dequant_f16
    with _on_device(p.device):
        _lib.check(fn(p.qweight.data_ptr(), p.rowmeta.data_ptr(), out.data_ptr(), p.N, p.K, _stream(out)),
                   "mxq_dequant_f16")
    return out


def dequant_bf16(p: PackedMXQ) -> torch.Tensor:
    """Dense bf16 [N, K] fake-quant weight: the fp32 s * (q - z) of ``dequant`` rounded once to bf16 (bit-identical to the
    reference's write-back into a bf16 layer)."""
    if not isinstance(p, PackedMXQ):
        raise ValueError("dequant_bf16 needs a PackedMXQ weight (mixed layout, exact or compact metadata)")
    _need_gpu(p.qweight)
    out = torch.empty((p.N, p.K), dtype=torch.bfloat16, device=p.device)
    with _on_device(p.device):
        _lib.check(_lib.load().mxq_dequant_bf16(p.qweight.data_ptr(), p.rowmeta.data_ptr(), out.data_ptr(), p.N, p.K,
                                                _layout_code(p), _stream(out)), "mxq_dequant_bf16")
    return out


def _dequant_t(p, dtype: torch.dtype) -> torch.Tensor:
    if isinstance(p, PackedUniform) and dtype == torch.bfloat16:
        raise ValueError("dequant_t_bf16 needs a PackedMXQ weight: bf16 is not built for uniform layouts")
    if not isinstance(p, (PackedMXQ, PackedUniform)):
        raise ValueError("dequant_t needs a PackedMXQ or PackedUniform weight")
    _need_gpu(p.qweight)
    out = torch.empty((p.K, p.N), dtype=dtype, device=p.device)
    lib = _lib.load()
    if isinstance(p, PackedUniform):
        with _on_device(p.device):
            _lib.check(lib.mxq_dequant_t_f16_layout(p.qweight.data_ptr(), p.rowmeta.data_ptr(), out.data_ptr(), p.N, p.K,
                                                    _layout_code(p), _stream(out)), "mxq_dequant_t_f16_layout")
        return out
    fn, what = (lib.mxq_dequant_t_bf16, "mxq_dequant_t_bf16") if dtype == torch.bfloat16 else (lib.mxq_dequant_t_f16, "mxq_dequant_t_f16")
    with _on_device(p.device):
        _lib.check(fn(p.qweight.data_ptr(), p.rowmeta.data_ptr(), out.data_ptr(), p.N, p.K, _layout_code(p), _stream(out)), what)
    return out


def dequant_t(p) -> torch.Tensor:
    """The transposed dense fp16 weight, a contiguous [K, N] tensor bit-identical to ``dequant(p).t().contiguous()``: the
    operand the dense kernels need for the input gradient (include/mxq_hip.h: mxq_dequant_t_f16; a PackedUniform:
    mxq_dequant_t_f16_layout, bit-identical to ``expand_uniform(p)[0].t()``)."""
    return _dequant_t(p, torch.float16)


def dequant_t_bf16(p: PackedMXQ) -> torch.Tensor:
    """``dequant_t`` in bf16: bit-identical to ``dequant_bf16(p).t().contiguous()``."""
    return _dequant_t(p, torch.bfloat16)


DENSE_VARIANTS = {"auto": 0, "dense128": 1, "dense256": 2}   # include/mxq_hip.h: mxq_dense_f16 variants


def _rows(x: torch.Tensor, names: tuple, dtype: torch.dtype, F: int, device: torch.device, out: Optional[torch.Tensor],
          F_out: int, late_error: Optional[str] = None):
    """The prologue of the wrappers that map a [..., F] tensor to a [..., F_out] one of the same dtype: checks x (dtype, last
    dimension, the weight's device), then raises `late_error` (a fault the caller found in its other arguments, reported after
    x's own), and returns x as contiguous [M, F] rows, `out` allocated or validated as [M, F_out], and M -- with M == 0 the
    caller launches nothing.  names: x's name, what it holds, the names of F and of F_out in the messages."""
    name, noun, f_name, out_name = names
    dt = str(dtype)[6:]
    if x.dtype != dtype:
        raise ValueError(f"{noun} must be {dt}, got {x.dtype}")
    if x.dim() < 1 or x.shape[-1] != F:
        raise ValueError(f"{f_name} mismatch: {name} has {x.shape[-1] if x.dim() else None}, weight has {F}")
    if x.device != device:
        raise ValueError(f"{name} and the packed weight live on different devices")
    if late_error:
        raise ValueError(late_error)
    x2 = x.reshape(-1, F).contiguous()
    M = x2.shape[0]
    if out is None:
        out = torch.empty((M, F_out), dtype=dtype, device=x.device)
    elif out.shape != (M, F_out) or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {dt} [tokens, {out_name}] tensor")
    return x2, out, M


def _linear_dense(dtype: torch.dtype, x: torch.Tensor, w16: torch.Tensor, out: Optional[torch.Tensor], variant: str) -> torch.Tensor:
    short, entry = ("bf16", "mxq_dense_bf16") if dtype == torch.bfloat16 else ("fp16", "mxq_dense_f16")
    _need_gpu(x, w16)
    if x.dtype != dtype or w16.dtype != dtype or w16.dim() != 2 or x.shape[-1] != w16.shape[1]:
        raise ValueError(f"expected {short} x [..., K] and {short} w16 [N, K]")
    if not w16.is_contiguous():
        raise ValueError("w16 must be contiguous")
    if variant not in DENSE_VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")
    N, K = w16.shape
    check_shape(N, K)
    x2, out, M = _rows(x, ("x", "activations", "K", "out_features"), dtype, K, x.device, out, N)   # (x checked above)
    if M:
        with _on_device(x.device):
            _lib.check(getattr(_lib.load(), entry)(x2.data_ptr(), w16.data_ptr(), out.data_ptr(), M, N, K,
                                                   DENSE_VARIANTS[variant], _stream(x2)), f"{entry}[{variant}]")
    return out.reshape(*x.shape[:-1], N)


def linear_dense(x: torch.Tensor, w16: torch.Tensor, out: Optional[torch.Tensor] = None, variant: str = "auto") -> torch.Tensor:
    """y = x @ w16.T on a dense fp16 [N, K] weight (e.g. ``dequant(p)``): the reference's ``nn.Linear`` on the fake-quant
    weight (mxq_quant/main.py:85) and the second half of the hoisted mode; fp32 accumulation, fp16 result.
    variant: "auto", "dense128" (256 x 128-tile kernel), "dense256" (256 x 256-tile kernel; K % 128 == 0)."""
    return _linear_dense(torch.float16, x, w16, out, variant)


def linear_dense_bf16(x: torch.Tensor, w16: torch.Tensor, out: Optional[torch.Tensor] = None, variant: str = "auto") -> torch.Tensor:
    """``linear_dense`` on bf16 operands: y = x @ w16.T for bf16 x [..., K] and a dense bf16 [N, K] weight (e.g.
    ``dequant_bf16(p)``), fp32 accumulation, bf16 result; the bf16 builds of the same two kernels, the same variants."""
    return _linear_dense(torch.bfloat16, x, w16, out, variant)


GEMM_PATHS = {"gemm": 0, "fused": 0, "gemm1": 1, "gemm8": 8, "gemm9": 9, "midm": 10, "gemm8h": 12, "gemm8h_split": 13, "gemm8h_slices": 14, "gemm8q_split": 16, "gemm8q_slices": 17, "gemm8n_split": 20, "gemm8n_slices": 21}   # include/mxq_hip.h: enum mxq_gemm_variant
# the paths of `linear` per layout code (_layout_code): the named kernels are the exact mixed layout's alone
_PATHS = ("auto", "gemm", "gemv", "skinny", "whole", "hoist", "fused")
_LAYOUT_PATHS = {0: frozenset(_PATHS + tuple(GEMM_PATHS)), 1: frozenset(_PATHS), 2: frozenset(_PATHS),
                 3: frozenset(_PATHS + ("gemm8",))}


def linear(x: torch.Tensor, p, out: Optional[torch.Tensor] = None, path: str = "auto") -> torch.Tensor:
    """y = x @ W.T for x [..., K] fp16 -> [..., N] fp16 (fp32 accumulation), W the dequantised weight of a PackedMXQ (mixed
    layout, exact or compact metadata) or a PackedUniform.

    path: "auto" (the library's own dispatch, mxq_linear_f16_auto: the schedules it picks are include/mxq_hip.h's enum
    mxq_linear_sched), "gemv" (<= 4 tokens), "skinny" (1..64 tokens), "hoist" (dequant hoisted out of the token loop),
    "gemm" (the fused kernel, hoisted from HOIST_MIN_TOKENS tokens on), "fused" (never hoisted), "whole" (fused kernel, whole
    tiles only: no stream-K split, so a tile's sums do not depend on the launch's token count).  On the mixed layout with
    exact metadata "gemm" / "fused" take the workspace (stream-K tail), and every kernel has a name (GEMM_PATHS,
    include/mxq_hip.h enum mxq_gemm_variant): "gemm1" (128x128 tile), "gemm8" (256x128 tile, wave-specialised, persistent,
    stream-K tail), "gemm9" (gemm8 splitting its tail whenever that is structurally possible: tests), "midm", "gemm8h" /
    "gemm8h_split" / "gemm8h_slices" (its 128-token build: tail split where it pays / always / K slices + combine launch),
    "gemm8q_*" (the 64-token build), "gemm8n_*" (the 128 x 64-tile build).  Compact metadata also has "gemm8" (= "fused")."""
    _need_gpu(x, p.qweight)
    if x.dtype != torch.float16:
        raise ValueError(f"activations must be float16 (W2/4 x A16), got {x.dtype}")
    if x.shape[-1] != p.K:
        raise ValueError(f"in_features mismatch: x has {x.shape[-1]}, weight has {p.K}")
    if x.device != p.qweight.device:
        raise ValueError("x and the packed weight live on different devices")
    flat = x.dim() == 2 and x.is_contiguous()          # (the usual call: no view objects made on the way in or out)
    x2 = x if flat else x.reshape(-1, p.K).contiguous()
    M = x2.shape[0]
    if out is None:
        out = torch.empty((M, p.N), dtype=torch.float16, device=x.device)
    elif out.shape != (M, p.N) or out.dtype != torch.float16 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float16 [tokens, out_features] tensor")
    if M == 0:
        return out.reshape(*x.shape[:-1], p.N)
    lib = _lib.load()
    lay = _layout_code(p)
    args = (x2.data_ptr(), p.qweight.data_ptr(), p.rowmeta.data_ptr(), out.data_ptr(), M, p.N, p.K, lay)
    st = _stream(x2)
    if path == "auto":
        # ONE C call for the whole dispatch; beyond the GEMV's token counts a workspace where the dispatch can use one
        # and -- under capture -- only as big as this launch needs, a scratch where it may hoist
        with _on_device(x.device):
            ws = None if M <= 4 else gemm_workspace(x2.device, stream=st, need=lib.mxq_linear_workspace_need(M, p.N, p.K, lay, 1))
            scratch = hoist_scratch(x2.device, lib.mxq_hoist_scratch_bytes(p.N, p.K)) if M >= HOIST_MIN_TOKENS else None
            _lib.check(lib.mxq_linear_f16_auto(*args, ws.data_ptr() if ws is not None else None,
                                               ws.numel() if ws is not None else 0,
                                               scratch.data_ptr() if scratch is not None else None,
                                               scratch.numel() if scratch is not None else 0, st),
                       "mxq_linear_f16_auto")
            if _CHECK_EVERY_CALL and ws is not None:
                workspace_status(x2.device)
        return out if flat else out.reshape(*x.shape[:-1], p.N)
    if path not in _LAYOUT_PATHS[lay]:
        raise ValueError(f"path {path!r} is not available for the {type(p).__name__} weight's layout")
    if path == "hoist" or (path == "gemm" and M >= HOIST_MIN_TOKENS):
        return linear_hoisted(x, p, out=out)
    ws = None
    with _on_device(x.device):
        if path == "gemv":
            rc = lib.mxq_gemv_f16_layout(*args, st)
        elif path == "skinny":
            rc = lib.mxq_skinny_f16(*args, st)
        elif path == "whole" or lay != 0:        # the fused kernel on whole tiles, no workspace
            rc = lib.mxq_gemm_f16_layout(*args, st)
        else:                                    # a named kernel of the mixed layout with exact metadata
            ws = gemm_workspace(x2.device, counters=path != "midm") if path != "gemm1" else None
            rc = lib.mxq_gemm_f16_ws(*args[:7], GEMM_PATHS[path], ws.data_ptr() if ws is not None else None,
                                     ws.numel() if ws is not None else 0, st)
        _lib.check(rc, f"linear[{path}]")
        if _CHECK_EVERY_CALL and ws is not None:
            workspace_status(x2.device)
    return out.reshape(*x.shape[:-1], p.N)


GRAD_INPUT_PATHS = ("auto", "single", "slices", "hoisted")


def grad_input_slices(M: int, N: int, K: int) -> int:
    """The number of N slices the "slices" path of ``linear_grad_input`` runs: the auto schedule's where it slices, else
    2 .. 4 (as many as fit the workspace; 1 where not even 2 fit)."""
    lib = _lib.load()
    need = lib.mxq_linear_grad_input_workspace_need(M, N, K, 0)
    if need:
        return (need - _lib.WS_HEAD_BYTES) // (M * K * 4)
    fit = (lib.mxq_gemm_workspace_bytes() - _lib.WS_HEAD_BYTES) // (M * K * 4)
    return max(1, min(4, fit))


# the C entry behind each (kind, path) of the input gradient (include/mxq_hip.h); "single" is the sliced entry run with one slice
_GRAD_INPUT_ENTRIES = {
    ("f16", "auto"): "mxq_linear_grad_input_f16_auto",
    ("f16", "single"): "mxq_linear_grad_input_f16_sliced",
    ("f16", "slices"): "mxq_linear_grad_input_f16_sliced",
    ("f16", "hoisted"): "mxq_linear_grad_input_f16_hoisted",
    ("bf16", "auto"): "mxq_linear_grad_input_bf16_auto",
    ("bf16", "single"): "mxq_linear_grad_input_bf16_sliced",
    ("bf16", "slices"): "mxq_linear_grad_input_bf16_sliced",
    ("bf16", "hoisted"): "mxq_linear_grad_input_bf16_hoisted",
    ("f16_layout", "auto"): "mxq_linear_grad_input_f16_layout_auto",
    ("f16_layout", "single"): "mxq_linear_grad_input_f16_layout_sliced",
    ("f16_layout", "slices"): "mxq_linear_grad_input_f16_layout_sliced",
    ("f16_layout", "hoisted"): "mxq_linear_grad_input_f16_layout_hoisted",
}


def _grad_input_launch(bf16: bool, args: tuple, M: int, p, lay: int, device: torch.device, st: int, path: str) -> int:
    """The C call behind ``linear_grad_input`` / ``linear_grad_input_bf16`` for one path; returns its code.  A PackedUniform
    (fp16 only) goes to the entries of the same names with ``_layout`` (include/mxq_hip.h)."""
    lib = _lib.load()
    uniform = isinstance(p, PackedUniform)
    entry = getattr(lib, _GRAD_INPUT_ENTRIES["f16_layout" if uniform else "bf16" if bf16 else "f16", path])
    ws_need = lib.mxq_linear_grad_input_layout_workspace_need if uniform else lib.mxq_linear_grad_input_workspace_need
    ptr = lambda t: (t.data_ptr(), t.numel()) if t is not None else (None, 0)   # noqa: E731
    if path == "auto":
        ws = gemm_workspace(device, counters=False, stream=st, need=ws_need(M, p.N, p.K, lay))
        hoist = M >= lib.mxq_linear_grad_input_hoist_min_tokens() and p.N % 64 == 0
        scratch = hoist_scratch(device, lib.mxq_hoist_scratch_bytes(p.N, p.K)) if hoist else None
        return entry(*args, *ptr(ws), *ptr(scratch), st)
    if path == "hoisted":
        if p.N % 64 != 0:
            raise ValueError(f"the hoisted input gradient needs out_features % 64 == 0, got {p.N}")
        scratch = hoist_scratch(device, lib.mxq_hoist_scratch_bytes(p.N, p.K))
        return entry(*args, *ptr(scratch), st)
    S = 1 if path == "single" else grad_input_slices(M, p.N, p.K)
    if path == "slices" and S < 2:
        raise ValueError(f"the slices of {M} tokens x {p.K} columns do not fit the workspace")
    ws = gemm_workspace(device, counters=False, stream=st) if S > 1 else None
    return entry(*args, S, *ptr(ws), st)


def _linear_grad_input(dtype: torch.dtype, what: str, dy: torch.Tensor, p, out: Optional[torch.Tensor], path: str) -> torch.Tensor:
    _need_gpu(dy, p.qweight)
    dy2, out, M = _rows(dy, ("dy", "gradients", "out_features", "in_features"), dtype, p.N, p.qweight.device, out, p.K,
                        None if path in GRAD_INPUT_PATHS else f"unknown path {path!r}")
    if M == 0:
        return out.reshape(*dy.shape[:-1], p.K)
    lay = _layout_code(p)
    args = (dy2.data_ptr(), p.qweight.data_ptr(), p.rowmeta.data_ptr(), out.data_ptr(), M, p.N, p.K, lay)
    st = _stream(dy2)
    with _on_device(dy.device):
        _lib.check(_grad_input_launch(dtype == torch.bfloat16, args, M, p, lay, dy2.device, st, path), f"{what}[{path}]")
    return out.reshape(*dy.shape[:-1], p.K)


def linear_grad_input(dy: torch.Tensor, p, out: Optional[torch.Tensor] = None, path: str = "auto") -> torch.Tensor:
    """dx = dy @ W for dy [..., N] fp16 -> [..., K] fp16 (fp32 accumulation), W the dequantised weight of a PackedMXQ
    (exact or compact metadata) or of a PackedUniform (``expand_uniform(p)[0]``): the input gradient of ``linear``, computed
    by the fused dequant kernel without materialising W (include/mxq_hip.h: mxq_linear_grad_input_f16; a PackedUniform:
    mxq_linear_grad_input_f16_layout and its siblings).

    path: "auto" (the library's dispatch, mxq_linear_grad_input_f16_auto: a workspace sized by
    mxq_linear_grad_input_workspace_need and, from mxq_linear_grad_input_hoist_min_tokens() tokens on, the per-device
    ``hoist_scratch`` the forward's hoisted mode uses -- stream-ordered, so sharing it is safe), "single" (one launch of whole
    tiles, no workspace), "slices" (the N reduction split into ``grad_input_slices`` slices: tests), "hoisted" (the transposing
    dequant into the scratch, then the dense kernels: bit-identical to ``linear_dense(dy, dequant_t(p))``; ValueError where
    out_features % 64 != 0)."""
    if not isinstance(p, (PackedMXQ, PackedUniform)):
        raise ValueError("linear_grad_input needs a PackedMXQ or PackedUniform weight")
    return _linear_grad_input(torch.float16, "linear_grad_input", dy, p, out, path)


BF16_PATHS = {"narrow": 1, "narrow_sliced": 2, "wide": 3, "wide_sliced": 4, "hoisted": 5}   # enum mxq_linear_bf16_sched


def linear_bf16(x: torch.Tensor, p: PackedMXQ, out: Optional[torch.Tensor] = None, path: str = "auto") -> torch.Tensor:
    """y = x @ W.T for x [..., K] bf16 -> [..., N] bf16 (fp32 accumulation), W = ``dequant_bf16(p)`` of a PackedMXQ (exact or
    compact metadata), computed by the fused dequant kernel without materialising W, or -- many tokens -- by the hoisted
    mode (include/mxq_hip.h: mxq_linear_bf16_auto).

    path: "auto" (the library's dispatch, with a workspace sized by mxq_linear_bf16_workspace_need and a scratch from
    mxq_linear_bf16_hoist_min_tokens() tokens on), or one schedule by name (BF16_PATHS, enum mxq_linear_bf16_sched: tests
    and A/B runs; a sliced schedule whose slabs do not fit the workspace raises ValueError)."""
    if not isinstance(p, PackedMXQ):
        raise ValueError("linear_bf16 needs a PackedMXQ weight (mixed layout, exact or compact metadata)")
    _need_gpu(x, p.qweight)
    x2, out, M = _rows(x, ("x", "activations", "in_features", "out_features"), torch.bfloat16, p.K, p.qweight.device, out, p.N,
                       None if path == "auto" or path in BF16_PATHS else f"unknown path {path!r}")
    if M == 0:
        return out.reshape(*x.shape[:-1], p.N)
    lib = _lib.load()
    lay = _layout_code(p)
    args = (x2.data_ptr(), p.qweight.data_ptr(), p.rowmeta.data_ptr(), out.data_ptr(), M, p.N, p.K, lay)
    st = _stream(x2)
    with _on_device(x.device):
        if path == "auto":
            hoist = M >= lib.mxq_linear_bf16_hoist_min_tokens()
            ws = gemm_workspace(x2.device, counters=False, stream=st,
                                need=lib.mxq_linear_bf16_workspace_need(M, p.N, p.K, lay, int(hoist)))
            scratch = hoist_scratch(x2.device, lib.mxq_hoist_scratch_bytes(p.N, p.K)) if hoist else None
            rc = lib.mxq_linear_bf16_auto(*args, ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                          scratch.data_ptr() if scratch is not None else None,
                                          scratch.numel() if scratch is not None else 0, st)
        else:
            ws = gemm_workspace(x2.device, counters=False, stream=st) if path.endswith("_sliced") else None
            scratch = hoist_scratch(x2.device, lib.mxq_hoist_scratch_bytes(p.N, p.K)) if path == "hoisted" else None
            rc = lib.mxq_linear_bf16_sched(*args, BF16_PATHS[path], ws.data_ptr() if ws is not None else None,
                                           ws.numel() if ws is not None else 0,
                                           scratch.data_ptr() if scratch is not None else None,
                                           scratch.numel() if scratch is not None else 0, st)
        _lib.check(rc, f"linear_bf16[{path}]")
    return out.reshape(*x.shape[:-1], p.N)


def linear_grad_input_bf16(dy: torch.Tensor, p: PackedMXQ, out: Optional[torch.Tensor] = None, path: str = "auto") -> torch.Tensor:
    """dx = dy @ W for dy [..., N] bf16 -> [..., K] bf16 (fp32 accumulation), W = ``dequant_bf16(p)``: the input gradient of
    ``linear_bf16`` (include/mxq_hip.h: mxq_linear_grad_input_bf16).  path as in ``linear_grad_input``."""
    if not isinstance(p, PackedMXQ):
        raise ValueError("linear_grad_input_bf16 needs a PackedMXQ weight (mixed layout, exact or compact metadata)")
    return _linear_grad_input(torch.bfloat16, "linear_grad_input_bf16", dy, p, out, path)


def linear_layout(x: torch.Tensor, p, out: Optional[torch.Tensor] = None, path: str = "gemm") -> torch.Tensor:
    """The former layout entry, kept as a name for bench.py: `linear` with its old default path "gemm"."""
    return linear(x, p, out=out, path=path)


def linear_fused(x: torch.Tensor, p: PackedMXQ, prologue: int = 0, norm_w: Optional[torch.Tensor] = None,
                 eps: float = 1e-5, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One-token quantised Linear with the neighbouring decoder-layer ops fused in (decode harness):
    prologue 0 none, 1 RMSNorm(x) * norm_w, 2 SwiGLU gate (x is [1, 2K] = gate | up);
    ``residual`` [1, N] is added to the result.  fp16 in / out, GEMV kernel."""
    _need_gpu(x, p.qweight, norm_w, residual)
    k_in = 2 * p.K if prologue == 2 else p.K
    if x.dtype != torch.float16 or x.numel() != k_in:
        raise ValueError(f"expected one fp16 token with {k_in} features")
    if prologue == 1 and (norm_w is None or norm_w.dtype != torch.float16 or norm_w.numel() != p.K):
        raise ValueError("RMSNorm prologue needs an fp16 weight of in_features elements")
    if residual is not None and (residual.dtype != torch.float16 or residual.numel() != p.N):
        raise ValueError("residual must be fp16 [1, out_features]")
    x = x.contiguous()
    out = torch.empty((1, p.N), dtype=torch.float16, device=x.device)
    lib = _lib.load()
    fused = lib.mxq_gemv_fused_f16_compact if p.compact else lib.mxq_gemv_fused_f16
    with _on_device(x.device):
        _lib.check(fused(x.data_ptr(), p.qweight.data_ptr(), p.rowmeta.data_ptr(), out.data_ptr(),
                         p.N, p.K, int(prologue), norm_w.data_ptr() if norm_w is not None else None,
                         float(eps), residual.contiguous().data_ptr() if residual is not None else None,
                         _stream(x)), "mxq_gemv_fused_f16")
    return out


def linear_swiglu(x: torch.Tensor, gate_up: PackedMXQ, norm_w: torch.Tensor, eps: float = 1e-5):
    """One token through RMSNorm -> gate | up -> SwiGLU in ONE launch (include/mxq_hip.h: mxq_gemv_swiglu_f16): ``gate_up`` is
    gate stacked on up ([2 I, K], ``concat_packed``).  Returns (act fp16 [1, I] in the kernels' staged order, act_sum f32
    [I / 16]) -- the input of ``linear_staged``; bit for bit what ``linear_fused(.., 1, norm_w)`` followed by the SwiGLU
    staging of ``linear_fused(.., 2)`` computes."""
    _need_gpu(x, gate_up.qweight, norm_w)
    if x.dtype != torch.float16 or x.numel() != gate_up.K or norm_w.dtype != torch.float16 or norm_w.numel() != gate_up.K:
        raise ValueError("expected one fp16 token and an fp16 RMSNorm weight of in_features elements")
    if gate_up.N % 32 != 0 or gate_up.K % 256 != 0:
        raise ValueError("the fused SwiGLU launch needs out_features % 32 == 0 (gate | up) and in_features % 256 == 0")
    inter = gate_up.N // 2
    x = x.contiguous()
    act = torch.empty((1, inter), dtype=torch.float16, device=x.device)
    act_sum = torch.empty(inter // 16, dtype=torch.float32, device=x.device)
    with _on_device(x.device):
        _lib.check(_lib.load().mxq_gemv_swiglu_f16(x.data_ptr(), gate_up.qweight.data_ptr(), gate_up.rowmeta.data_ptr(),
                                                   act.data_ptr(), act_sum.data_ptr(), gate_up.N, gate_up.K, norm_w.data_ptr(),
                                                   float(eps), int(gate_up.compact), _stream(x)), "mxq_gemv_swiglu_f16")
    return act, act_sum


def linear_staged(act: torch.Tensor, act_sum: torch.Tensor, p: PackedMXQ, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = residual + W . act for a staged row from ``linear_swiglu`` (mxq_gemv_staged_f16)."""
    _need_gpu(act, act_sum, p.qweight, residual)
    if act.dtype != torch.float16 or act.numel() != p.K or act_sum.dtype != torch.float32 or act_sum.numel() != p.K // 16:
        raise ValueError("expected a staged fp16 row of in_features elements and its in_features / 16 fp32 group sums")
    if residual is not None and (residual.dtype != torch.float16 or residual.numel() != p.N):
        raise ValueError("residual must be fp16 [1, out_features]")
    out = torch.empty((1, p.N), dtype=torch.float16, device=act.device)
    with _on_device(act.device):
        _lib.check(_lib.load().mxq_gemv_staged_f16(act.data_ptr(), act_sum.data_ptr(), p.qweight.data_ptr(), p.rowmeta.data_ptr(),
                                                   out.data_ptr(), p.N, p.K,
                                                   residual.contiguous().data_ptr() if residual is not None else None,
                                                   int(p.compact), _stream(act)), "mxq_gemv_staged_f16")
    return out


# ------------------------------------------------------------------------------------------------
# uniform layouts of the BASELINE config-5 sweep (W2A16 / W4A16 arms next to the mixed layout)
# ------------------------------------------------------------------------------------------------
LAYOUTS = {"mixed": 0, "w2g16": 1, "w4row": 2}
# The ONE table of module / file format versions (QuantLinear's ``fmt[0]``, checkpoint.py): version -> (layout name, compact
# metadata).  Not the C layout code (include/mxq_hip.h MXQ_LAYOUT_*), where 3 is the mixed layout with compact metadata.
FORMAT_VERSIONS = {1: ("mixed", False), 2: ("mixed", True), 3: ("w2g16", False), 4: ("w4row", False)}


def format_version(layout: str, compact_meta: bool = False) -> int:
    """The module format version of a layout name (FORMAT_VERSIONS read backwards); ValueError for a pair that has none."""
    for ver, key in FORMAT_VERSIONS.items():
        if key == (layout, bool(compact_meta)):
            return ver
    if layout in LAYOUTS and compact_meta:
        raise ValueError(f"compact metadata exists for the mixed layout only, not for {layout!r}")
    raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")


def layout_qweight_bytes(N: int, K: int, layout: str, compact_meta: bool = False) -> int:
    """Bytes of the block array of a [N, K] weight in a layout (mxq_qweight_bytes_layout)."""
    check_shape(N, K)
    format_version(layout, compact_meta)
    return _lib.load().mxq_qweight_bytes_layout(N, K, 3 if compact_meta else LAYOUTS[layout])


@dataclass
class PackedUniform:
    """W2G16 / W4ROW packed weight (csrc/mxq_format.h); same [N/16][K/64] block grid as PackedMXQ."""
    qweight: torch.Tensor
    rowmeta: torch.Tensor
    N: int
    K: int
    layout: str

    @property
    def device(self):
        return self.qweight.device

    def nbytes(self) -> int:
        return self.qweight.numel() * 4 + self.rowmeta.numel() * 4

    def bits_per_weight(self) -> float:
        return 8.0 * self.nbytes() / (self.N * self.K)


def quantize_pack_uniform(W: torch.Tensor, layout: str) -> PackedUniform:
    """Quantise W [N, K] with ``Quantizer(bits=2, group 16)`` ("w2g16") or ``Quantizer(bits=4, per row)``
    ("w4row"), both with the 4-bit second-order scale coding (reference lib/quantizer.py:61-147)."""
    _need_gpu(W)
    if layout not in ("w2g16", "w4row"):
        raise ValueError("layout must be 'w2g16' or 'w4row'")
    if W.dim() != 2 or W.dtype not in _TORCH2CODE:
        raise ValueError("weight must be a 2-D fp16 / bf16 / fp32 tensor")
    N, K = W.shape
    check_shape(N, K)
    W = W.contiguous()
    lib = _lib.load()
    nbytes = lib.mxq_qweight_bytes_layout(N, K, LAYOUTS[layout])
    p = PackedUniform(torch.empty(nbytes // 4, dtype=torch.int32, device=W.device),
                      torch.empty((N, 4), dtype=torch.float32, device=W.device), N, K, layout)
    with _on_device(W.device):
        _lib.check(lib.mxq_quantize_pack_layout(W.data_ptr(), _TORCH2CODE[W.dtype], p.qweight.data_ptr(),
                                                p.rowmeta.data_ptr(), N, K, LAYOUTS[layout], _stream(W)),
                   "mxq_quantize_pack_layout")
    return p


def expand_uniform(p: PackedUniform, codes: bool = True):
    """(fp16 [N, K] dequantised weight, dict of integer codes / parameters or None)."""
    N, K, dev = p.N, p.K, p.qweight.device
    w16 = torch.empty((N, K), dtype=torch.float16, device=dev)
    out = None
    ptrs = [None] * 5
    if codes:
        G = K // 16 if p.layout == "w2g16" else 1
        out = dict(codes=torch.empty((N, K), dtype=torch.uint8, device=dev),
                   sc=torch.empty((N, G), dtype=torch.uint8, device=dev),
                   zero=torch.empty((N, G), dtype=torch.float32, device=dev),
                   qs=torch.empty((N // 16, G), dtype=torch.float32, device=dev),
                   qz=torch.empty((N // 16, G), dtype=torch.float32, device=dev))
        ptrs = [out[k].data_ptr() for k in ("codes", "sc", "zero", "qs", "qz")]
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.mxq_expand_layout(p.qweight.data_ptr(), p.rowmeta.data_ptr(), w16.data_ptr(), *ptrs, N, K,
                                         LAYOUTS[p.layout], _stream(w16)), "mxq_expand_layout")
    return w16, out


def dequant_uniform(p: PackedUniform) -> torch.Tensor:
    """Dense fp16 [N, K] weight of a PackedUniform: ``expand_uniform(p)[0]`` without the code tensors."""
    _need_gpu(p.qweight)
    return expand_uniform(p, codes=False)[0]


# ------------------------------------------------------------------------------------------------
# calibration statistics of the per-layer layout choice (lib/layout_search.py; csrc/quant_error.hip)
# ------------------------------------------------------------------------------------------------
def col_moment(x: torch.Tensor, moment: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum over all rows of x[..., K]^2 as fp32 [K] (include/mxq_hip.h: mxq_col_moment): the diagonal of the Hessian sum of
    x x^T of a Linear's input.  x fp16 / bf16 / fp32 on the GPU, in_features % 64 == 0.  ``moment`` (fp32 [K], contiguous, on
    x's device): accumulated in place and returned.  Deterministic: fp32 sums in a fixed order, no atomics."""
    _need_gpu(x, moment)
    if x.dtype not in _TORCH2CODE:
        raise ValueError(f"unsupported activation dtype {x.dtype}")
    if x.dim() < 1 or x.shape[-1] <= 0 or x.shape[-1] % 64 != 0:
        raise ValueError(f"col_moment needs x [..., K] with K % 64 == 0, got {tuple(x.shape)}")
    K = x.shape[-1]
    if moment is None:
        out = torch.empty(K, dtype=torch.float32, device=x.device)
    elif moment.dtype != torch.float32 or tuple(moment.shape) != (K,) or not moment.is_contiguous() or moment.device != x.device:
        raise ValueError("moment must be a contiguous float32 [in_features] tensor on x's device")
    else:
        out = moment
    x2 = x.reshape(-1, K).contiguous()
    if x2.shape[0] == 0:
        return out.zero_() if moment is None else out
    with _on_device(x.device):
        _lib.check(_lib.load().mxq_col_moment(x2.data_ptr(), _TORCH2CODE[x.dtype], x2.shape[0], K,
                                              moment.data_ptr() if moment is not None else None, out.data_ptr(), _stream(x2)),
                   "mxq_col_moment")
    return out


def quant_error(W: torch.Tensor, p, col_weight: Optional[torch.Tensor] = None, with_ref: bool = False):
    """err_rows fp32 [N]: err_rows[n] = sum_k c[k] (W[n, k] - W'[n, k])^2, W' the fp16 weight ``dequant(p)`` would write, c =
    ``col_weight`` (fp32 [K]; None: ones) -- with c = E[x_k^2] (``col_moment`` / tokens) the diagonal-Hessian estimate of the
    squared output error of the Linear, row by row.  ``with_ref``: also ref_rows[n] = sum_k c[k] W[n, k]^2, returned as
    (err_rows, ref_rows).  One fused kernel (include/mxq_hip.h: mxq_quant_error): W' is never written to memory.
    W: fp16 / bf16 / fp32 [N, K] on the GPU, the shape of ``p`` (a PackedMXQ, exact or compact, or a PackedUniform)."""
    if not isinstance(p, (PackedMXQ, PackedUniform)):
        raise ValueError("quant_error needs a PackedMXQ or PackedUniform weight")
    _need_gpu(W, p.qweight, col_weight)
    if W.dim() != 2 or W.dtype not in _TORCH2CODE:
        raise ValueError("weight must be a 2-D fp16 / bf16 / fp32 tensor")
    if tuple(W.shape) != (p.N, p.K):
        raise ValueError(f"weight is {tuple(W.shape)}, the packed weight [{p.N}, {p.K}]")
    if W.device != p.qweight.device:
        raise ValueError("W and the packed weight live on different devices")
    if col_weight is not None:
        if col_weight.dtype != torch.float32 or col_weight.numel() != p.K or col_weight.device != W.device:
            raise ValueError("col_weight must be a float32 tensor of in_features entries on W's device")
        col_weight = col_weight.reshape(-1).contiguous()
    W = W.contiguous()
    err = torch.empty(p.N, dtype=torch.float32, device=W.device)
    ref = torch.empty(p.N, dtype=torch.float32, device=W.device) if with_ref else None
    with _on_device(W.device):
        _lib.check(_lib.load().mxq_quant_error(W.data_ptr(), _TORCH2CODE[W.dtype], p.qweight.data_ptr(), p.rowmeta.data_ptr(),
                                               col_weight.data_ptr() if col_weight is not None else None, err.data_ptr(),
                                               ref.data_ptr() if ref is not None else None, p.N, p.K, _layout_code(p),
                                               _stream(W)), "mxq_quant_error")
    return (err, ref) if with_ref else err
