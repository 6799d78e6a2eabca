"""Tensor-level front-end of the C ABI (include/qsae.h): torch supplies device memory and the
current HIP stream, libqsae_hip.so does the work.  Every function requires CUDA (ROCm)
tensors and raises otherwise -- there is no CPU path in this package.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import sys
import threading
import weakref
from typing import Callable, NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID, check  # noqa: F401


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_tensor_device(fn):
    """Run `fn` with the device of its first tensor argument current: the C ABI (like any HIP library) launches on the
    current device, and a model moved to cuda:1 must not launch on cuda:0 because that is what the thread last used."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        for a in args:
            if isinstance(a, torch.Tensor):
                if a.is_cuda and a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return wrapper


class _HipEventPair:
    """Two timing events for qsae_profile_sweep_events, created / read / destroyed through libqsae_hip.so itself
    (qsae_profile_event_*): the runtime that records them is the one that made them."""

    def __init__(self):
        lib = _lib.load()
        self._lib = lib
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            check(lib.qsae_profile_event_create(C.byref(e)))

    def elapsed_ms(self):
        ms = C.c_float(0.0)
        return ms.value if self._lib.qsae_profile_event_elapsed_ms(self.a, self.b, C.byref(ms)) == 0 else None

    def destroy(self):
        for e in (self.a, self.b):
            self._lib.qsae_profile_event_destroy(e)


class _KernelTimer:
    """Optional HIP-event brackets (used by bench.py to time the dominant kernel live inside the timed region).
    `encode_dense` launches are bracketed here; the candidate sweep is launched inside the library, which records a
    pair handed to it per call (sweep_pairs).  All events sit on the stream the kernel is launched on and are read only
    after the region has been synchronised."""

    def __init__(self):
        self.enabled = False
        self.sweep = False          # hand an event pair to every fused / prefilter call
        self._events = {}
        self._sweep_pairs = []

    def reset(self):
        self._events = {}
        for p in self._sweep_pairs:
            p.destroy()
        self._sweep_pairs = []

    def bracket(self, name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self._events.setdefault(name, []).append((a, b))
        return a, b

    def mean_ms(self, name):
        ev = self._events.get(name)
        if not ev:
            return None
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev)

    def arm_sweep(self):
        """Called right before a library call that contains a candidate sweep."""
        if self.sweep:
            p = _HipEventPair()
            self._sweep_pairs.append(p)
            check(_lib.load().qsae_profile_sweep_events(p.a, p.b))

    def sweep_mean_ms(self):
        """-> (mean ms per sweep launch or None, launches); the region must have been synchronised."""
        ms = [m for m in (p.elapsed_ms() for p in self._sweep_pairs) if m is not None]
        return (sum(ms) / len(ms) if ms else None), len(ms)


kernel_timer = _KernelTimer()


def sweep_timing(enable: bool) -> None:
    """Time the candidate-sweep launch of every following fused / prefilter call (HIP events on the launch stream)."""
    kernel_timer.sweep = bool(enable)


def sweep_timing_collect(H: int):
    """-> (mean ms per sweep launch or None, launches, fraction of the encoder FLOPs per launch)."""
    ms, n = kernel_timer.sweep_mean_ms()
    return ms, n, float(_lib.load().qsae_profile_sweep_flop_fraction(H))


def _dev(t: torch.Tensor, name: str, dtype=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: quantizedsae_amd runs on MI355X only; tensor is on {t.device} "
                           "(no CPU fallback exists)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    _dev(t, name)
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _p(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


# ---- encoder ------------------------------------------------------------------------------
@_on_tensor_device
def kperm_rows(src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K-interleaved copy of a [rows, K] fp32 matrix (K % 8 == 0); see qsae_kperm_rows."""
    src = _f32c(src, "src")
    rows, K = src.shape
    if out is None:
        out = torch.empty_like(src)
    check(_lib.load().qsae_kperm_rows(_p(src), rows, K, _p(out), _stream()))
    return out


@_on_tensor_device
def encode_dense(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], act: int = ACT_NONE,
                 out: Optional[torch.Tensor] = None, kperm: bool = False) -> torch.Tensor:
    """kperm=True: x and W are already K-interleaved (kperm_rows)."""
    x, W = _f32c(x, "x"), _f32c(W, "W")
    B, D = x.shape
    H = W.shape[0]
    if W.shape[1] != D:
        raise ValueError(f"W is {tuple(W.shape)}, expected [H, {D}]")
    b = _f32c(bias, "bias") if bias is not None else None
    if out is None:
        out = torch.empty((B, H), dtype=torch.float32, device=x.device)
    ev = kernel_timer.bracket("encode_dense") if kernel_timer.enabled else None
    if ev:
        ev[0].record()
    fn = _lib.load().qsae_encode_dense_kperm if kperm else _lib.load().qsae_encode_dense
    check(fn(_p(x), _p(W), _p(b), B, D, H, act, _p(out), out.stride(0) if B else H, _stream()))
    if ev:
        ev[1].record()
    return out


def encode_dense_emu_supported(D: int) -> bool:
    return D > 0 and D % 64 == 0


@_on_tensor_device
def emu_pack_w(W: torch.Tensor):
    """-> (Wc fp16 [H, 3 D], meta2 fp32 [2]) for encode_dense_emu (once per checkpoint)."""
    W = _f32c(W, "W")
    H, D = W.shape
    Wc = torch.empty((H, 3 * D), dtype=torch.float16, device=W.device)
    meta2 = torch.zeros((2,), dtype=torch.float32, device=W.device)
    check(_lib.load().qsae_emu_pack_w(_p(W), H, D, _p(Wc), _p(meta2), _stream()))
    return Wc, meta2


@_on_tensor_device
def encode_dense_emu(x: torch.Tensor, Wc: torch.Tensor, meta2: torch.Tensor, bias: Optional[torch.Tensor],
                     act: int = ACT_NONE) -> torch.Tensor:
    """encode_dense at fp32 accuracy (not bit-exactness) on the fp16 matrix pipe: see qsae_encode_dense_emu."""
    x = _f32c(x, "x")
    B, D = x.shape
    H = Wc.shape[0]
    b = _f32c(bias, "bias") if bias is not None else None
    out = torch.empty((B, H), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    need = int(lib.qsae_encode_dense_emu_workspace_bytes(B, D)) if B > 0 else 1
    if need == 0:
        raise ValueError("shape not supported by the emulated encoder (D % 64 == 0)")
    ws = _workspace(x.device, need)
    check(lib.qsae_encode_dense_emu(_p(x), _p(Wc), _p(meta2), _p(b), B, D, H, act, _p(out), H, _p(ws), ws.numel(), _stream()))
    return out


@_on_tensor_device
def encode_bits(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """uint32-packed z bits [B, ceil(H/32)] (returned as int32 tensor)."""
    x, W = _f32c(x, "x"), _f32c(W, "W")
    B, D = x.shape
    H = W.shape[0]
    b = _f32c(bias, "bias") if bias is not None else None
    words = (H + 31) // 32
    z = torch.empty((B, words), dtype=torch.int32, device=x.device)
    check(_lib.load().qsae_encode_bits(_p(x), _p(W), _p(b), B, D, H, _p(z), words, _stream()))
    return z


# The two fp16 routes to the z bits: kind -> (workspace sizer, blocking, submit and finish entry point, refusal text).
_BITS_FP16 = {
    "prefilter": ("qsae_encode_bits_prefilter_workspace_bytes", "qsae_encode_bits_prefilter", "qsae_encode_bits_prefilter_submit",
                  "qsae_encode_bits_prefilter_finish", "shape not supported by the fp16 candidate sweep"),
    "band": ("qsae_encode_bits_band_workspace_bytes", "qsae_encode_bits_band", "qsae_encode_bits_band_submit",
             "qsae_encode_bits_band_finish", "shape not supported by the fp16 band classification"),
}


def _encode_bits_fp16_supported(kind: str, B: int, D: int, H: int) -> bool:
    return B > 0 and int(getattr(_lib.load(), _BITS_FP16[kind][0])(B, D, H)) > 0


def _encode_bits_fp16_operands(kind: str, x, W, bias):
    """-> (x, W, bias checked, B, D, H, workspace bytes) for the entry points of ``kind``; refuses a shape they do not take."""
    x, W = _f32c(x, "x"), _f32c(W, "W")
    B, D = x.shape
    H = W.shape[0]
    b = _f32c(bias, "bias") if bias is not None else None
    need = int(getattr(_lib.load(), _BITS_FP16[kind][0])(B, D, H)) if B > 0 else 1
    if need == 0:
        raise ValueError(_BITS_FP16[kind][4])
    return x, W, b, B, D, H, need


def _encode_bits_fp16_cargs(x, W, b, Wq, meta, B, D, H, ws):
    """-> (C arguments up to workspace_bytes, tensors they point into, zbits)."""
    words = (H + 31) // 32
    z = torch.empty((B, words), dtype=torch.int32, device=x.device)
    return (_p(x), _p(W), _p(b), _p(Wq), _p(meta), B, D, H, _p(z), words, _p(ws), ws.numel()), (x, W, b, Wq, meta, ws), z


@_on_tensor_device
def _encode_bits_fp16(kind: str, x, W, bias, Wq, meta) -> Tuple[torch.Tensor, int]:
    x, W, b, B, D, H, need = _encode_bits_fp16_operands(kind, x, W, bias)
    if B == 0:
        return torch.empty((0, (H + 31) // 32), dtype=torch.int32, device=x.device), 0
    cargs, _keep, z = _encode_bits_fp16_cargs(x, W, b, Wq, meta, B, D, H, _workspace(x.device, need))
    flagged = C.c_int(0)
    kernel_timer.arm_sweep()
    check(getattr(_lib.load(), _BITS_FP16[kind][1])(*cargs, C.byref(flagged), _stream()))
    return z, int(flagged.value)


def encode_bits_prefilter_supported(B: int, D: int, H: int) -> bool:
    return _encode_bits_fp16_supported("prefilter", B, D, H)


def encode_bits_band_supported(B: int, D: int, H: int) -> bool:
    return _encode_bits_fp16_supported("band", B, D, H)


def encode_bits_prefilter(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], Wq: torch.Tensor,
                          meta: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """z bits identical to encode_bits, from the fp16 candidate sweep + exact re-evaluation of the latents near the
    cutoff.  Returns (zbits int32 [B, ceil(H/32)], rows that went through the exact dense kernel)."""
    return _encode_bits_fp16("prefilter", x, W, bias, Wq, meta)


def encode_bits_band(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], Wq: torch.Tensor,
                     meta: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """z bits identical to encode_bits for DENSE activations: every latent classified by an fp16 MFMA pass, the
    uncertainty band around the cutoff re-evaluated exactly.  Returns (zbits, rows that went through the exact kernel)."""
    return _encode_bits_fp16("band", x, W, bias, Wq, meta)


@_on_tensor_device
def encode_bits_prefilter_submit(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], Wq: torch.Tensor,
                                 meta: torch.Tensor, slot: int = 0, band: bool = False, owner: int = 0) -> "PendingForward":
    """The two-call form of encode_bits_prefilter (qsae_encode_bits_prefilter_submit / _finish) or, with ``band``, of
    encode_bits_band: ``finish()`` returns the z bits; ``flagged_rows`` of the handle is the number of rows that went
    through the exact dense kernel."""
    kind = "band" if band else "prefilter"
    x, W, b, B, D, H, need = _encode_bits_fp16_operands(kind, x, W, bias)
    slot = (owner, slot)
    _claim_slot(x.device, slot)
    cargs, keep, z = _encode_bits_fp16_cargs(x, W, b, Wq, meta, B, D, H, _workspace(x.device, need, slot, "pending"))
    lib = _lib.load()
    return _submit(getattr(lib, _BITS_FP16[kind][2]), getattr(lib, _BITS_FP16[kind][3]), cargs, keep, z, x.device, slot)


@_on_tensor_device
def topk_rows(latent: torch.Tensor, k: int, zero_rest: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """In-place on `latent` when zero_rest.  Returns (idx int32 [B,k], val f32 [B,k])."""
    _dev(latent, "latent", torch.float32)
    if latent.dim() != 2 or latent.stride(1) != 1:
        raise ValueError("latent must be a 2-D tensor with unit inner stride")
    B, H = latent.shape
    idx = torch.empty((B, k), dtype=torch.int32, device=latent.device)
    val = torch.empty((B, k), dtype=torch.float32, device=latent.device)
    if zero_rest:
        _latent_pool_forget(latent)
    check(_lib.load().qsae_topk_rows(_p(latent), latent.stride(0) if B else H, B, H, k, _p(idx), _p(val),
                                     1 if zero_rest else 0, _stream()))
    return idx, val


_workspaces = collections.OrderedDict()     # (device, stream handle, kind, slot) -> uint8 tensor, least recently used first
#: scratch buffers kept per device (each is ~0.7 GB at the headline shape): the blocking calls of one stream need one,
#: every batch in flight another; streams / threads that have gone leave theirs behind until they fall off this list
WORKSPACE_CACHE_PER_DEVICE = 6
_busy_slots = {}                            # (device, stream handle, slot) -> PendingForward that owns the slot


def _workspace(device: torch.device, nbytes: int, slot: int = 0, kind: str = "call") -> torch.Tensor:
    """Scratch for one call in flight: one buffer per (device, stream, kind, slot).  Two streams never share one (their
    kernels would write the same candidate lists), and a buffer that has to grow is simply replaced: the old block goes
    back to the caching allocator, which reuses memory in the order of the stream it was allocated on -- the same
    stream every user of this buffer ran on.  kind "call" = the blocking entry points (whose use of the buffer ends with
    the call's last kernel), kind "pending" = submit / finish pairs, which own their buffer until finish() -- a blocking
    call between the two must not touch it -- with ``slot`` separating batches in flight together on one stream.
    The cache keeps the WORKSPACE_CACHE_PER_DEVICE most recently used buffers of a device (release_workspaces()
    drops all)."""
    dev = device.index if device.index is not None else torch.cuda.current_device()
    key = (dev, torch.cuda.current_stream(device).cuda_stream, kind, slot)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    _workspaces.move_to_end(key)
    mine = [k for k in _workspaces if k[0] == dev]
    for k in mine[:max(0, len(mine) - WORKSPACE_CACHE_PER_DEVICE)]:
        ref = _busy_slots.get((k[0], k[1], k[3])) if k[2] == "pending" else None
        if ref is not None and ref() is not None:
            continue                        # a batch in flight still owns it
        del _workspaces[k]                  # (the block returns to the caching allocator, stream-ordered)
    return ws


def release_workspaces() -> None:
    """Drop every cached scratch buffer (they are re-created on demand).  Buffers of batches still in flight stay alive
    through their PendingForward handles.  The pool of dropped dense latents (below) is emptied too."""
    _workspaces.clear()
    with _latent_pool_lock:
        del _latent_pool[:]


# ---- dropped dense latents, reused -------------------------------------------
# A [B, H] latent that a forward-in-one-call prefilter entry point allocated and wrote is +0 everywhere except at the k
# positions per row listed in that call's idx.  Once its caller has dropped it, the next call of the same shape on the same
# stream takes it back and has the library erase those B k entries (qsae_recycle.h) in place of writing B H zeros.
#: False: every call allocates its latent with torch.empty and has all its zeros written (no record is kept either)
LATENT_RECYCLE = True
#: records kept per device, the oldest dropped first; each holds a [B, H] latent (8.6 GB at the headline shape) and its idx
LATENT_POOL_PER_DEVICE = 4
_LatentRecord = collections.namedtuple("_LatentRecord", "key dense idx dense_version idx_version")
_latent_pool = []                               # _LatentRecord, oldest first; key = (device, stream handle, B, H, k)
_latent_pool_lock = threading.Lock()
#: lookups of the pool since import: a hit took a dropped latent back, a miss fell through to torch.empty
latent_pool_stats = {"hits": 0, "misses": 0}
_latent_holder_baseline = None


def _latent_holders(rec):
    """The counters that together see every other holder of rec.dense: a second Python reference, a view or slice, a
    detached alias, .numpy(), a DLPack capsule -- and, by the last one, the storage object itself (torch hands out one
    Python object per storage, so holding it moves none of the first three)."""
    dense = rec.dense
    storage = dense.untyped_storage()
    return (sys.getrefcount(dense), dense._use_count(), torch._C._storage_Use_Count(storage._cdata), sys.getrefcount(storage))


def _latent_unheld(rec) -> bool:
    """Whether the record is the only holder of its latent: the counters stand where they stand for a fresh tensor held
    the same way (measured once, not assumed)."""
    global _latent_holder_baseline
    if _latent_holder_baseline is None:
        _latent_holder_baseline = _latent_holders(_LatentRecord(None, torch.empty((1, 1)), None, 0, 0))
    return _latent_holders(rec) == _latent_holder_baseline


def _latent_pool_take(key):
    """-> (dense, idx) of the first record of ``key`` whose latent nobody else holds and whose tensors torch has not seen
    written since, removed from the pool; None when there is none.  A record torch has seen written is dropped."""
    with _latent_pool_lock:
        edited = [r for r in _latent_pool if r.dense._version != r.dense_version or r.idx._version != r.idx_version]
        if edited:
            _latent_pool[:] = [r for r in _latent_pool if not any(r is e for e in edited)]
        for i, rec in enumerate(_latent_pool):
            if rec.key == key and _latent_unheld(rec):
                del _latent_pool[i]
                latent_pool_stats["hits"] += 1
                return rec.dense, rec.idx
        latent_pool_stats["misses"] += 1
    return None


def _latent_pool_register(key, dense, idx) -> None:
    """``dense`` [B, H] is finished: zeros and the entries listed in ``idx``.  Called when the last kernel that writes it has
    been enqueued."""
    try:
        rec = _LatentRecord(key, dense, idx, dense._version, idx._version)
    except RuntimeError:                        # inference tensors carry no version counter: an edit would go unseen
        return
    with _latent_pool_lock:
        _latent_pool.append(rec)
        mine = [r for r in _latent_pool if r.key[0] == key[0]]
        drop = mine[:max(0, len(mine) - LATENT_POOL_PER_DEVICE)]
        if drop:
            _latent_pool[:] = [r for r in _latent_pool if not any(r is d for d in drop)]


def _latent_pool_forget(t: torch.Tensor) -> None:
    """``t`` is about to be written through its raw pointer, which torch's version counter does not see: whatever record
    shares its storage no longer describes it."""
    if not _latent_pool:
        return
    ptr = t.untyped_storage().data_ptr()
    with _latent_pool_lock:
        _latent_pool[:] = [r for r in _latent_pool if r.dense.untyped_storage().data_ptr() != ptr]


def _recycled(name: str, tail) -> str:
    """The library symbol for a call with a stale list: the qsaer_* form of qsae_recycle.h."""
    return "qsaer_" + name[len("qsae_"):] if tail else name


def encode_topk_supported(B: int, D: int, H: int, k: int) -> bool:
    """Whether encode_topk / encode_topk_latent run this shape (fused form for large batches, chunked form otherwise)."""
    return int(_lib.load().qsae_encode_topk_workspace_bytes(B, D, H, k)) > 0


def _encode_topk_workspace(lib, B: int, D: int, H: int, k: int) -> int:
    need = int(lib.qsae_encode_topk_workspace_bytes(B, D, H, k))
    if need == 0 and B > 0:
        raise ValueError(f"encode_topk: shape B={B}, D={D}, H={H}, k={k} is outside what the kernels run (fused form: "
                         "B >= 2048, 8192 <= H <= 65536; otherwise H <= 32768; H % 4 == 0, D % 4 == 0, k <= 256)")
    return need


@_on_tensor_device
def encode_topk(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], k: int, kperm: bool = False):
    """kperm=True: x and W are already K-interleaved (kperm_rows)."""
    x, W = _f32c(x, "x"), _f32c(W, "W")
    B, D = x.shape
    H = W.shape[0]
    b = _f32c(bias, "bias") if bias is not None else None
    lib = _lib.load()
    need = _encode_topk_workspace(lib, B, D, H, k)
    ws = _workspace(x.device, need)
    idx = torch.empty((B, k), dtype=torch.int32, device=x.device)
    val = torch.empty((B, k), dtype=torch.float32, device=x.device)
    fn = lib.qsae_encode_topk_kperm if kperm else lib.qsae_encode_topk
    kernel_timer.arm_sweep()
    check(fn(_p(x), _p(W), _p(b), B, D, H, k, _p(idx), _p(val), _p(ws), ws.numel(), _stream()))
    return idx, val


@_on_tensor_device
def encode_topk_latent(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], k: int, kperm: bool = False):
    """-> (idx, val, dense latent [B,H]); the dense tensor is zero-filled inside the encoder sweep."""
    x, W = _f32c(x, "x"), _f32c(W, "W")
    B, D = x.shape
    H = W.shape[0]
    b = _f32c(bias, "bias") if bias is not None else None
    lib = _lib.load()
    need = _encode_topk_workspace(lib, B, D, H, k)
    ws = _workspace(x.device, need)
    idx = torch.empty((B, k), dtype=torch.int32, device=x.device)
    val = torch.empty((B, k), dtype=torch.float32, device=x.device)
    dense = torch.empty((B, H), dtype=torch.float32, device=x.device)
    kernel_timer.arm_sweep()
    check(lib.qsae_encode_topk_latent(_p(x), _p(W), _p(b), B, D, H, k, _p(idx), _p(val), _p(dense), H,
                                      1 if kperm else 0, _p(ws), ws.numel(), _stream()))
    return idx, val, dense


@_on_tensor_device
def prefilter_pack_w(W: torch.Tensor, bias: Optional[torch.Tensor]):
    """-> (Wq fp16 [H, D], meta fp32 [4]) for encode_topk_prefilter (once per checkpoint)."""
    W = _f32c(W, "W")
    H, D = W.shape
    b = _f32c(bias, "bias") if bias is not None else None
    Wq = torch.empty((H, D), dtype=torch.float16, device=W.device)
    meta = torch.zeros((4,), dtype=torch.float32, device=W.device)
    check(_lib.load().qsae_prefilter_pack_w(_p(W), _p(b), H, D, _p(Wq), _p(meta), _stream()))
    return Wq, meta


def prefilter_supported(B: int, D: int, H: int, k: int) -> bool:
    return int(_lib.load().qsae_encode_topk_prefilter_workspace_bytes(B, D, H, k)) > 0


@_on_tensor_device
def encode_topk_prefilter(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], Wq: torch.Tensor,
                          meta: torch.Tensor, k: int, want_dense: bool = True, dense_out: Optional[torch.Tensor] = None,
                          spec_rows: int = 0, info: Optional[dict] = None):
    """fp16-prefiltered encoder + exact top-k (+ dense latent): results identical to encode_topk_latent.
    ``dense_out``: optional [B, >=H] fp32 buffer (row stride a multiple of 4) that receives the dense latent.
    ``spec_rows``: flagged rows the device recomputes while the host waits for their count (see qsae.h).
    ``info``: a dict that receives ``flagged_rows`` (rows that went through the exact fallback kernels)."""
    x, W = _f32c(x, "x"), _f32c(W, "W")
    B, D = x.shape
    H = W.shape[0]
    b = _f32c(bias, "bias") if bias is not None else None
    lib = _lib.load()
    need = int(lib.qsae_encode_topk_prefilter_workspace_bytes(B, D, H, k))
    if need == 0:
        raise ValueError("shape not supported by the fp16 prefilter")
    ws = _workspace(x.device, need)
    idx = torch.empty((B, k), dtype=torch.int32, device=x.device)
    val = torch.empty((B, k), dtype=torch.float32, device=x.device)
    if dense_out is not None:
        _dev(dense_out, "dense_out", torch.float32)
        if dense_out.dim() != 2 or dense_out.shape[0] != B or dense_out.shape[1] < H or dense_out.stride(1) != 1:
            raise ValueError("dense_out must be a [B, >=H] fp32 tensor with unit column stride")
        dense, ld = dense_out, dense_out.stride(0)
        _latent_pool_forget(dense_out)
    else:
        dense = torch.empty((B, H), dtype=torch.float32, device=x.device) if want_dense else None
        ld = H
    flagged = C.c_int(0)
    kernel_timer.arm_sweep()
    check(lib.qsae_encode_topk_prefilter(_p(x), _p(W), _p(b), _p(Wq), _p(meta), B, D, H, k, _p(idx), _p(val),
                                         _p(dense), ld, _p(ws), ws.numel(), int(spec_rows), C.byref(flagged), _stream()))
    if info is not None:
        info["flagged_rows"] = int(flagged.value)
    return idx, val, (dense[:, :H] if dense_out is not None else dense)


def _decode_prefilter_args(x, W, bias, Wq, meta, k, decoder, dec_bias, want_dense, slot, kind):
    """Argument tuple shared by the forward-in-one-call entry points.  ``decoder`` = ("packed", packed uint8 [H, row_bytes],
    n_bits, step) or ("table", fp32 [H, D], scale).
    -> (cargs, keep, outs, pool key or None, tail): with a dense latent and LATENT_RECYCLE the latent is a dropped one of the
    pool where there is one -- ``tail`` = (stale_idx, stale_k), the arguments the qsaer_* form of the call takes behind the
    stream, else () -- and the caller registers (pool key, dense, idx) once the call has fully finished."""
    x, W = _f32c(x, "x"), _f32c(W, "W")
    B, D = x.shape
    H = W.shape[0]
    b = _f32c(bias, "bias") if bias is not None else None
    db = _f32c(dec_bias, "dec_bias") if dec_bias is not None else None
    if decoder[0] == "packed":
        dict_t = _dev(decoder[1], "packed", torch.uint8)
        dargs = (_p(dict_t), int(decoder[2]), float(decoder[3]))
    else:
        dict_t = _f32c(decoder[1], "table")
        if tuple(dict_t.shape) != (H, D):
            raise ValueError(f"table is {tuple(dict_t.shape)}, expected [{H}, {D}]")
        dargs = (_p(dict_t), float(decoder[2]))
    need = int(_lib.load().qsae_encode_topk_prefilter_workspace_bytes(B, D, H, k))
    if need == 0:
        raise ValueError("shape not supported by the fp16 prefilter")
    ws = _workspace(x.device, need, slot, kind)
    idx = torch.empty((B, k), dtype=torch.int32, device=x.device)
    val = torch.empty((B, k), dtype=torch.float32, device=x.device)
    dense = stale = pool_key = None
    if want_dense and LATENT_RECYCLE:
        dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
        pool_key = (dev, torch.cuda.current_stream(x.device).cuda_stream, B, H, k)
        dense, stale = _latent_pool_take(pool_key) or (None, None)
    if want_dense and dense is None:
        dense = torch.empty((B, H), dtype=torch.float32, device=x.device)
    recon = torch.empty((B, D), dtype=torch.float32, device=x.device)
    cargs = (_p(x), _p(W), _p(b), _p(Wq), _p(meta), B, D, H, k) + dargs + (_p(db), _p(idx), _p(val), _p(dense), H, _p(recon),
                                                                          _p(ws), ws.numel())
    keep = (x, W, b, Wq, meta, dict_t, db, ws, stale)   # referenced by the pointers above
    return cargs, keep, (idx, val, dense, recon), pool_key, ((_p(stale), k) if stale is not None else ())


# library symbols of the forward-in-one-call entry points, by the kind of decoder description
_PREFILTER_FORWARD = {"packed": "qsae_binary_forward_prefilter", "table": "qsae_table_forward_prefilter"}
_PREFILTER_SUBMIT = {"packed": ("qsae_prefilter_submit", "qsae_prefilter_finish"),
                     "table": ("qsae_prefilter_submit_table", "qsae_prefilter_finish_table")}


@_on_tensor_device
def _forward_prefilter(x, W, bias, Wq, meta, k, decoder, dec_bias, want_dense, spec_rows, info):
    cargs, keep, outs, pool_key, tail = _decode_prefilter_args(x, W, bias, Wq, meta, k, decoder, dec_bias, want_dense, 0, "call")
    flagged = C.c_int(0)
    kernel_timer.arm_sweep()
    fn = getattr(_lib.load(), _recycled(_PREFILTER_FORWARD[decoder[0]], tail))
    check(fn(*cargs, int(spec_rows), C.byref(flagged), _stream(), *tail))
    if pool_key is not None:
        _latent_pool_register(pool_key, outs[2], outs[0])
    if info is not None:
        info["flagged_rows"] = int(flagged.value)
    return outs


def binary_forward_prefilter(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], Wq: torch.Tensor,
                             meta: torch.Tensor, k: int, packed: torch.Tensor, n_bits: int, step: float,
                             dec_bias: Optional[torch.Tensor], want_dense: bool = True, spec_rows: int = 0,
                             info: Optional[dict] = None):
    """encode_topk_prefilter + decode_binary_sparse in one call (rows are decoded by the refinement kernel as it
    ranks them): (idx, val, dense latent or None, reconstruction), bit-identical to the two separate calls."""
    return _forward_prefilter(x, W, bias, Wq, meta, k, ("packed", packed, n_bits, step), dec_bias, want_dense, spec_rows, info)


def table_forward_prefilter(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], Wq: torch.Tensor,
                            meta: torch.Tensor, k: int, table: torch.Tensor, scale: float,
                            dec_bias: Optional[torch.Tensor], want_dense: bool = True, spec_rows: int = 0,
                            info: Optional[dict] = None):
    """encode_topk_prefilter + decode_table_sparse in one call (fp32 dictionary rows [H, D]: the Baseline decoder, the
    soft integers of an unpolarised BinarySAE): (idx, val, dense latent or None, reconstruction), bit-identical to the
    two separate calls."""
    return _forward_prefilter(x, W, bias, Wq, meta, k, ("table", table, scale), dec_bias, want_dense, spec_rows, info)


class PendingForward:
    """A batch whose main kernels are queued (*_submit).  ``finish()`` waits for the 4-byte count of rows that need
    the exact fallback -- by then the GPU is usually busy with the NEXT batch's kernels -- enqueues that fallback ON THE
    STREAM THE BATCH WAS SUBMITTED ON and returns the outputs, which must not be read before ``finish()`` has returned.
    The handle owns its workspace slot from submit to finish: a second submit into the same slot raises, and the
    blocking entry points use buffers of their own, so nothing between the two calls can disturb the lists the fallback
    reads.  Not safe to share between threads."""

    def __init__(self, finish_fn, cargs, keep, outs, word, event, device, stream, slot_key, latent_record=None):
        self._finish_fn, self._cargs, self._keep, self._outs = finish_fn, cargs, keep, outs
        self._word, self._event, self._device, self._stream, self._slot_key = word, event, device, stream, slot_key
        self._latent_record = latent_record             # (pool key, dense, idx): registered once finish() has enqueued the rest
        self.flagged_rows = None
        _busy_slots[slot_key] = weakref.ref(self)       # (weak: a dropped handle must still be collected)

    def _release(self):
        ref = _busy_slots.get(self._slot_key)
        if ref is not None and ref() in (self, None):
            del _busy_slots[self._slot_key]
        self._cargs = self._keep = self._latent_record = None

    def finish(self):
        if self._cargs is None:
            return self._outs
        self._event.synchronize()                      # the count has landed in the pinned word
        self.flagged_rows = int(self._word.item())
        try:
            with torch.cuda.device(self._device), torch.cuda.stream(self._stream):
                check(self._finish_fn(*self._cargs, self.flagged_rows, _stream()))
            if self._latent_record is not None:
                _latent_pool_register(*self._latent_record)
        finally:
            self._release()
        return self._outs

    def __del__(self):
        # dropped without finish(): the asynchronous 4-byte copy may still be pending -- the pinned word must outlive it
        try:
            if self._cargs is not None:
                self._event.synchronize()
                self._release()
        except Exception:
            pass


def _submit(submit_fn, finish_fn, cargs, keep, outs, device, slot, tail=(), latent_record=None):
    """``tail``: arguments of submit_fn behind the stream (the finish function takes none); ``latent_record``: what
    finish() registers with the pool of dropped latents."""
    stream = torch.cuda.current_stream(device)
    slot_key = (device.index if device.index is not None else torch.cuda.current_device(), stream.cuda_stream, slot)
    word = torch.zeros((1,), dtype=torch.int32).pin_memory()
    kernel_timer.arm_sweep()
    check(submit_fn(*cargs, C.c_void_p(word.data_ptr()), _stream(), *tail))
    ev = torch.cuda.Event()
    ev.record(stream)
    return PendingForward(finish_fn, cargs, keep, outs, word, ev, device, stream, slot_key, latent_record)


def _claim_slot(device, slot):
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream, slot)
    ref = _busy_slots.get(key)
    if ref is not None and ref() is None:
        del _busy_slots[key]                # its handle is gone (collected without finish)
        ref = None
    if ref is not None:
        raise RuntimeError(f"submit: slot {slot[-1] if isinstance(slot, tuple) else slot} of this stream still holds a batch whose finish() / result() has not been "
                           "called; batches in flight together need different slot numbers")


@_on_tensor_device
def _forward_prefilter_submit(x, W, bias, Wq, meta, k, decoder, dec_bias, want_dense, slot, owner) -> PendingForward:
    slot = (owner, slot)            # slots are per owner (module): two models on one stream do not share workspaces
    _claim_slot(x.device, slot)
    cargs, keep, outs, pool_key, tail = _decode_prefilter_args(x, W, bias, Wq, meta, k, decoder, dec_bias, want_dense, slot,
                                                               "pending")
    lib = _lib.load()
    submit_name, finish_name = _PREFILTER_SUBMIT[decoder[0]]
    return _submit(getattr(lib, _recycled(submit_name, tail)), getattr(lib, finish_name), cargs, keep, outs, x.device, slot,
                   tail=tail, latent_record=(pool_key, outs[2], outs[0]) if pool_key is not None else None)


def binary_forward_prefilter_submit(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], Wq: torch.Tensor,
                                    meta: torch.Tensor, k: int, packed: torch.Tensor, n_bits: int, step: float,
                                    dec_bias: Optional[torch.Tensor], want_dense: bool = True,
                                    slot: int = 0, owner: int = 0) -> PendingForward:
    """The two-call form of binary_forward_prefilter (qsae_prefilter_submit / _finish): nothing in here waits for the
    GPU, so the caller can submit batch i+1 before it finishes batch i.  Batches in flight together on one stream
    need different ``slot`` numbers (each slot is a workspace of its own); finish them in submission order."""
    return _forward_prefilter_submit(x, W, bias, Wq, meta, k, ("packed", packed, n_bits, step), dec_bias, want_dense, slot,
                                     owner)


def table_forward_prefilter_submit(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], Wq: torch.Tensor,
                                   meta: torch.Tensor, k: int, table: torch.Tensor, scale: float,
                                   dec_bias: Optional[torch.Tensor], want_dense: bool = True,
                                   slot: int = 0, owner: int = 0) -> PendingForward:
    """The two-call form of table_forward_prefilter (qsae_prefilter_submit_table / _finish_table)."""
    return _forward_prefilter_submit(x, W, bias, Wq, meta, k, ("table", table, scale), dec_bias, want_dense, slot, owner)


@_on_tensor_device
def densify(idx: torch.Tensor, val: torch.Tensor, H: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _dev(idx, "idx", torch.int32)
    _dev(val, "val", torch.float32)
    B, k = idx.shape
    if out is None:
        out = torch.empty((B, H), dtype=torch.float32, device=idx.device)
    else:
        _latent_pool_forget(out)
    check(_lib.load().qsae_densify(_p(idx.contiguous()), _p(val.contiguous()), B, k, H, _p(out),
                                   out.stride(0) if B else H, _stream()))
    return out


# ---- BinarySAE dictionary -----------------------------------------------------------------
def binary_row_bytes(D: int, n_bits: int) -> int:
    r = int(_lib.load().qsae_binary_row_bytes(D, n_bits))
    if r < 0:
        check(r)
    return r


@_on_tensor_device
def pack_binary(logits: torch.Tensor, D: int, n_bits: int, want_polarize: bool = True, want_soft_gap: bool = False):
    """-> (packed uint8 [H, row_bytes], polarize_sum float64 0-d tensor or None[, soft_gap float32 0-d tensor]).
    soft_gap = max |soft integer - hard integer| over the dictionary (see qsae_pack_binary)."""
    logits = _f32c(logits, "logits")
    H = logits.shape[0]
    if logits.shape[1] != D * n_bits:
        raise ValueError(f"logits is {tuple(logits.shape)}, expected [H, {D * n_bits}]")
    packed = torch.empty((H, binary_row_bytes(D, n_bits)), dtype=torch.uint8, device=logits.device)
    pol = torch.zeros((), dtype=torch.float64, device=logits.device) if want_polarize else None
    gap = torch.zeros((), dtype=torch.float32, device=logits.device) if want_soft_gap else None
    check(_lib.load().qsae_pack_binary(_p(logits), H, D, n_bits, _p(packed), _p(pol), _p(gap), _stream()))
    return (packed, pol, gap) if want_soft_gap else (packed, pol)


@_on_tensor_device
def unpack_binary(packed: torch.Tensor, D: int, n_bits: int) -> torch.Tensor:
    _dev(packed, "packed", torch.uint8)
    H = packed.shape[0]
    out = torch.empty((H, D), dtype=torch.float32, device=packed.device)
    check(_lib.load().qsae_unpack_binary(_p(packed), H, D, n_bits, _p(out), _stream()))
    return out


@_on_tensor_device
def binary_soft_table(logits: torch.Tensor, D: int, n_bits: int) -> torch.Tensor:
    logits = _f32c(logits, "logits")
    H = logits.shape[0]
    out = torch.empty((H, D), dtype=torch.float32, device=logits.device)
    check(_lib.load().qsae_binary_soft_table(_p(logits), H, D, n_bits, _p(out), _stream()))
    return out


@_on_tensor_device
def decode_binary_sparse(idx, val, packed, D: int, n_bits: int, step: float, bias=None) -> torch.Tensor:
    _dev(idx, "idx", torch.int32)
    _dev(val, "val", torch.float32)
    _dev(packed, "packed", torch.uint8)
    B, k = idx.shape
    H = packed.shape[0]
    b = _f32c(bias, "bias") if bias is not None else None
    recon = torch.empty((B, D), dtype=torch.float32, device=idx.device)
    check(_lib.load().qsae_decode_binary_sparse(_p(idx.contiguous()), _p(val.contiguous()), B, k, _p(packed), H, D,
                                                n_bits, float(step), _p(b), _p(recon), _stream()))
    return recon


@_on_tensor_device
def decode_table_sparse(idx, val, table: torch.Tensor, scale: float = 1.0, bias=None) -> torch.Tensor:
    _dev(idx, "idx", torch.int32)
    _dev(val, "val", torch.float32)
    table = _f32c(table, "table")
    B, k = idx.shape
    H, D = table.shape
    b = _f32c(bias, "bias") if bias is not None else None
    recon = torch.empty((B, D), dtype=torch.float32, device=idx.device)
    check(_lib.load().qsae_decode_table_sparse(_p(idx.contiguous()), _p(val.contiguous()), B, k, _p(table), H, D,
                                               float(scale), _p(b), _p(recon), _stream()))
    return recon


# ---- ternary ---------------------------------------------------------------------------------
@_on_tensor_device
def pack_ternary(w: torch.Tensor) -> torch.Tensor:
    """decoder.weight [D, H] -> 2-bit codes int32 [D, ceil(H/16)]."""
    w = _f32c(w, "w")
    D, H = w.shape
    codes = torch.empty((D, (H + 15) // 16), dtype=torch.int32, device=w.device)
    check(_lib.load().qsae_pack_ternary(_p(w), D, H, _p(codes), _stream()))
    return codes


@_on_tensor_device
def decode_ternary_dense(h: torch.Tensor, codes: torch.Tensor, D: int) -> torch.Tensor:
    _dev(h, "h", torch.float32)
    B, H = h.shape
    recon = torch.empty((B, D), dtype=torch.float32, device=h.device)
    check(_lib.load().qsae_decode_ternary_dense(_p(h), h.stride(0) if B else H, B, H, _p(codes), D, _p(recon),
                                                _stream()))
    return recon


# ---- dense decoders on the bf16 matrix pipe ----------------------------------------------------
def split_dec_supported(B: int, H: int, D: int) -> bool:
    return bool(_lib.load().qsae_split_dec_supported(int(B), int(H), int(D)))


@_on_tensor_device
def expand_codes_bf16(codes: torch.Tensor, D: int, H: int) -> torch.Tensor:
    """2-bit codes [D, ceil(H/16)] (pack_ternary / pack_matryoshka) -> the bf16 dictionary image the split decoders
    stream (opaque, 2 H D bytes; once per checkpoint)."""
    _dev(codes, "codes", torch.int32)
    lib = _lib.load()
    nbytes = int(lib.qsae_expand_codes_bf16_bytes(D, H))
    if nbytes == 0:
        raise ValueError("shape not supported by the bf16 split decoders (D == 512, H % 64 == 0)")
    tq = torch.empty((nbytes // 2,), dtype=torch.bfloat16, device=codes.device)
    check(lib.qsae_expand_codes_bf16(_p(codes.contiguous()), D, H, _p(tq), _stream()))
    return tq


@_on_tensor_device
def decode_ternary_dense_split(h: torch.Tensor, tq: torch.Tensor, D: int) -> torch.Tensor:
    """decode_ternary_dense from three exact bf16 terms of h on v_mfma_f32_32x32x16_bf16 (fp32 accumulation)."""
    _dev(h, "h", torch.float32)
    B, H = h.shape
    recon = torch.empty((B, D), dtype=torch.float32, device=h.device)
    check(_lib.load().qsae_decode_ternary_dense_split(_p(h), h.stride(0) if B else H, B, H, _p(tq), D, _p(recon), _stream()))
    return recon


@_on_tensor_device
def split_scale_bf16(scale: torch.Tensor) -> torch.Tensor:
    """scale [H] (pack_matryoshka) -> the three bf16 terms of 2 * scale, [3, H] bfloat16."""
    scale = _f32c(scale, "scale")
    H = scale.shape[0]
    s3 = torch.empty((3, H), dtype=torch.bfloat16, device=scale.device)
    check(_lib.load().qsae_split_scale_bf16(_p(scale), H, _p(s3), _stream()))
    return s3


@_on_tensor_device
def decode_matryoshka_split(zbits: torch.Tensor, H: int, D: int, n_bits: int, tq, s3, bias, allow_bias: bool, sizes=None):
    """decode_matryoshka on the bf16 matrix pipe: -> (levels f32 [n_bits, B, D], l0_counts int64 [n_bits])."""
    _dev(zbits, "zbits", torch.int32)
    B = zbits.shape[0]
    levels = torch.empty((n_bits, B, D), dtype=torch.float32, device=zbits.device)
    counts = torch.zeros((n_bits,), dtype=torch.int64, device=zbits.device)
    b = _f32c(bias, "bias") if bias is not None else None
    keep, sp = _sizes_arg(sizes, n_bits)
    check(_lib.load().qsae_decode_matryoshka_split(_p(zbits), zbits.stride(0) if B else (H + 31) // 32, B, H, D, n_bits, sp,
                                                   _p(tq), _p(s3), _p(b), 1 if allow_bias else 0, _p(levels), _p(counts),
                                                   _stream()))
    return levels, counts


# ---- matryoshka ------------------------------------------------------------------------------
def matryoshka_sizes(H: int, n_bits: int):
    arr = (C.c_int32 * n_bits)()
    check(_lib.load().qsae_matryoshka_sizes(H, n_bits, C.cast(arr, C.c_void_p)))
    return [int(v) for v in arr]


def _sizes_arg(sizes, n_bits):
    if sizes is None:
        return None, C.c_void_p(0)
    if len(sizes) != n_bits:
        raise ValueError("level sizes must have n_bits entries")
    arr = (C.c_int32 * n_bits)(*[int(s) for s in sizes])
    return arr, C.cast(arr, C.c_void_p)


@_on_tensor_device
def pack_matryoshka(w: torch.Tensor, wm: torch.Tensor, n_bits: int, abs_range: float, sizes=None):
    """-> (codes int32 [D, ceil(H/16)] of S/2, scale fp32 [H])."""
    w, wm = _f32c(w, "w"), _f32c(wm, "wm")
    H, D = w.shape
    codes = torch.empty((D, (H + 15) // 16), dtype=torch.int32, device=w.device)
    scale = torch.empty((H,), dtype=torch.float32, device=w.device)
    keep, sp = _sizes_arg(sizes, n_bits)
    check(_lib.load().qsae_pack_matryoshka(_p(w), _p(wm), H, D, n_bits, float(abs_range), sp, _p(codes), _p(scale),
                                           _stream()))
    return codes, scale


@_on_tensor_device
def decode_matryoshka(zbits: torch.Tensor, H: int, D: int, n_bits: int, codes, scale, bias, allow_bias: bool,
                      sizes=None):
    """-> (levels f32 [n_bits, B, D], l0_counts int64 [n_bits])."""
    _dev(zbits, "zbits", torch.int32)
    B = zbits.shape[0]
    levels = torch.empty((n_bits, B, D), dtype=torch.float32, device=zbits.device)
    counts = torch.zeros((n_bits,), dtype=torch.int64, device=zbits.device)
    b = _f32c(bias, "bias") if bias is not None else None
    keep, sp = _sizes_arg(sizes, n_bits)
    check(_lib.load().qsae_decode_matryoshka(_p(zbits), zbits.stride(0) if B else (H + 31) // 32, B, H, D, n_bits,
                                             sp, _p(codes), _p(scale), _p(b), 1 if allow_bias else 0, _p(levels),
                                             _p(counts), _stream()))
    return levels, counts


@_on_tensor_device
def pack_matryoshka_rows(w: torch.Tensor, wm: torch.Tensor) -> torch.Tensor:
    """-> codes_rows int32 [H, ceil(D/8)]: the dictionary in hidden-major order (4-bit fields) for decode_matryoshka_sparse."""
    w, wm = _f32c(w, "w"), _f32c(wm, "wm")
    H, D = w.shape
    codes = torch.empty((H, (D + 7) // 8), dtype=torch.int32, device=w.device)
    check(_lib.load().qsae_pack_matryoshka_rows(_p(w), _p(wm), H, D, _p(codes), _stream()))
    return codes


def decode_matryoshka_sparse_supported(D: int) -> bool:
    return D in (64, 128, 256, 512, 1024)


@_on_tensor_device
def decode_matryoshka_sparse(zbits: torch.Tensor, H: int, D: int, n_bits: int, codes_rows, scale, bias,
                             allow_bias: bool, sizes=None):
    """decode_matryoshka on the active units only (same outputs)."""
    _dev(zbits, "zbits", torch.int32)
    B = zbits.shape[0]
    levels = torch.empty((n_bits, B, D), dtype=torch.float32, device=zbits.device)
    counts = torch.zeros((n_bits,), dtype=torch.int64, device=zbits.device)
    b = _f32c(bias, "bias") if bias is not None else None
    keep, sp = _sizes_arg(sizes, n_bits)
    check(_lib.load().qsae_decode_matryoshka_sparse(_p(zbits), zbits.stride(0) if B else (H + 31) // 32, B, H, D,
                                                    n_bits, sp, _p(codes_rows), _p(scale), _p(b),
                                                    1 if allow_bias else 0, _p(levels), _p(counts), _stream()))
    return levels, counts


@_on_tensor_device
def pack_bits_gt(dense: torch.Tensor, thr: float) -> torch.Tensor:
    """int32-packed bits [B, ceil(H/32)] of (dense > thr)."""
    _dev(dense, "dense", torch.float32)
    if dense.stride(1) != 1:
        dense = dense.contiguous()
    B, H = dense.shape
    words = (H + 31) // 32
    z = torch.empty((B, words), dtype=torch.int32, device=dense.device)
    check(_lib.load().qsae_pack_bits_gt(_p(dense), dense.stride(0) if B else H, B, H, float(thr), _p(z), words,
                                        _stream()))
    return z


# ---- small elementwise steps ---------------------------------------------------------------------
@_on_tensor_device
def residual_update(residual: torch.Tensor, recon: torch.Tensor, scale: float = 2.0) -> torch.Tensor:
    """(residual - recon) * scale, each operation rounded separately (sae/residual_quantized.py:67)."""
    residual, recon = _f32c(residual, "residual"), _f32c(recon, "recon")
    if residual.shape != recon.shape:
        raise ValueError("residual and recon must have the same shape")
    out = torch.empty_like(residual)
    check(_lib.load().qsae_residual_update(_p(residual), _p(recon), residual.numel(), float(scale), _p(out), _stream()))
    return out


@_on_tensor_device
def threshold_ge(pre: torch.Tensor, cutoff: float) -> torch.Tensor:
    """1.0 where pre >= cutoff else 0.0 (sae/binary_latent.py:21-24 with the fp32 cutoff of sigmoid >= 0.5)."""
    pre = _f32c(pre, "pre")
    out = torch.empty_like(pre)
    check(_lib.load().qsae_threshold_ge(_p(pre), pre.numel(), float(cutoff), _p(out), _stream()))
    return out


@_on_tensor_device
def scale_bias_rows(acc: torch.Tensor, scale: float, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """scale * acc + bias over the rows of a [B, D] tensor, multiply and add rounded separately (sae/binary.py:38)."""
    acc = _f32c(acc, "acc")
    B, D = acc.shape
    b = _f32c(bias, "bias") if bias is not None else None
    out = torch.empty_like(acc)
    check(_lib.load().qsae_scale_bias_rows(_p(acc), B, D, float(scale), _p(b), _p(out), _stream()))
    return out


# ---- metric ------------------------------------------------------------------------------------
@_on_tensor_device
def sq_err_sum(recon: torch.Tensor, x: torch.Tensor, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """acc (float64 0-d device tensor) += sum((recon - x)^2); returns acc (no host sync)."""
    recon, x = _f32c(recon, "recon"), _f32c(x, "x")
    if recon.shape != x.shape:
        raise ValueError("recon and x must have the same shape")
    if acc is None:
        acc = torch.zeros((), dtype=torch.float64, device=x.device)
    check(_lib.load().qsae_sq_err_sum(_p(recon), _p(x), recon.numel(), _p(acc), _stream()))
    return acc


# ---- consumers of the sparse latent (activation statistics) ---------------------------------------------
@_on_tensor_device
def activation_counts(idx: torch.Tensor, val: Optional[torch.Tensor], H: int,
                      counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """counts[h] += #rows whose entry h is active (val > 0; every listed entry when val is None).  int64 [H]."""
    _dev(idx, "idx", torch.int32)
    B, k = idx.shape
    if val is not None:
        _dev(val, "val", torch.float32)
    if counts is None:
        counts = torch.zeros((H,), dtype=torch.int64, device=idx.device)
    check(_lib.load().qsae_activation_counts(_p(idx.contiguous()), _p(val.contiguous()) if val is not None else None,
                                             B, k, H, _p(counts), _stream()))
    return counts


@_on_tensor_device
def activation_counts_bits(zbits: torch.Tensor, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """counts[32 w + j] += popcount over rows of bit j of word w.  zbits int32 [B, words]; int64 [32 * words]."""
    _dev(zbits, "zbits", torch.int32)
    B, words = zbits.shape
    if counts is None:
        counts = torch.zeros((32 * words,), dtype=torch.int64, device=zbits.device)
    check(_lib.load().qsae_activation_counts_bits(_p(zbits), zbits.stride(0) if B else words, B, 32 * words, _p(counts),
                                                  _stream()))
    return counts


@_on_tensor_device
def coactivation_sparse(idx: torch.Tensor, val: Optional[torch.Tensor], H: int,
                        coact: Optional[torch.Tensor] = None) -> torch.Tensor:
    """coact[a, c] += #rows in which units a and c are both active (mask^T @ mask).  int32 [H, H]."""
    _dev(idx, "idx", torch.int32)
    B, k = idx.shape
    if val is not None:
        _dev(val, "val", torch.float32)
    if coact is None:
        coact = torch.zeros((H, H), dtype=torch.int32, device=idx.device)
    check(_lib.load().qsae_coactivation_sparse(_p(idx.contiguous()), _p(val.contiguous()) if val is not None else None,
                                               B, k, H, _p(coact), coact.stride(0), _stream()))
    return coact


@_on_tensor_device
def coactivation_bits(zbits: torch.Tensor, H: int, index: Optional[torch.Tensor] = None,
                      coact: Optional[torch.Tensor] = None) -> torch.Tensor:
    """coact[u(p), u(q)] += #rows in which packed positions p and q are both set (mask^T @ mask on the int8 matrix
    pipe, from the packed bits).  zbits int32 [B, words]; ``index`` (int32 / int64 [32 * words]) maps a packed position
    to its unit, -1 = pad slot (masked, never written); None = identity (32 * words <= H).  int32 [H, H].
    A contiguous int32 ``index`` is passed through as it is; an int64 one is converted on every call, so a caller that
    accumulates over many batches converts its map once and passes the int32 tensor (analysis.py does).  ``zbits`` may
    be a column slice of a wider packed tensor (row stride > words)."""
    _dev(zbits, "zbits", torch.int32)
    B, words = zbits.shape
    if zbits.stride(1) != 1:
        zbits = zbits.contiguous()
    if index is not None:
        if index.dtype not in (torch.int32, torch.int64):
            raise TypeError("index: expected int32 or int64")
        if index.numel() != 32 * words:
            raise ValueError(f"index: expected {32 * words} entries (one per packed position), got {index.numel()}")
        index = _dev(index.to(torch.int32).contiguous(), "index", torch.int32)
    if coact is None:
        coact = torch.zeros((H, H), dtype=torch.int32, device=zbits.device)
    else:
        _dev(coact, "coact", torch.int32)
        if coact.dim() != 2 or coact.shape[0] != H or coact.shape[1] < H or coact.stride(1) != 1:
            raise ValueError("coact: expected an int32 [H, >= H] matrix with unit column stride")
    lib = _lib.load()
    need = int(lib.qsae_coactivation_bits_workspace_bytes(B, 32 * words)) if B > 0 else 0
    ws = _workspace(zbits.device, max(need, 1))
    check(lib.qsae_coactivation_bits(_p(zbits), zbits.stride(0) if B else words, B, 32 * words, _p(index), int(H),
                                     _p(coact), coact.stride(0), _p(ws), ws.numel(), _stream()))
    return coact


def _partners_state(partners: Optional[torch.Tensor], P: int, device) -> torch.Tensor:
    """the partner-set state int32 [P, >= P / 32] (int32 words stand in for uint32), allocated zeroed when None"""
    if partners is None:
        return torch.zeros((P, P // 32), dtype=torch.int32, device=device)
    _dev(partners, "partners", torch.int32)
    if partners.dim() != 2 or partners.shape[0] != P or partners.shape[1] < P // 32 or partners.stride(1) != 1:
        raise ValueError(f"partners: expected an int32 [{P}, >= {P // 32}] matrix with unit column stride")
    return partners


def _packed_index_arg(index: Optional[torch.Tensor], nbits: int) -> Optional[torch.Tensor]:
    if index is None:
        return None
    if index.dtype not in (torch.int32, torch.int64):
        raise TypeError("index: expected int32 or int64")
    if index.numel() != nbits:
        raise ValueError(f"index: expected {nbits} entries (one per packed position), got {index.numel()}")
    return _dev(index.to(torch.int32).contiguous(), "index", torch.int32)


@_on_tensor_device
def coactivation_partners_bits(zbits: torch.Tensor, index: Optional[torch.Tensor] = None,
                               partners: Optional[torch.Tensor] = None) -> torch.Tensor:
    """partners |= "packed positions p and q were set in the same row": bit q & 31 of word q >> 5 of row p, diagonal
    included (qsae_coactivation_partners_bits; the main loop of coactivation_bits with a one-bit epilogue).  zbits int32
    [B, words], a column slice of a wider tensor is read in place; ``index`` (int32 / int64 [32 * words]) only masks:
    positions with index < 0 are inert.  The state is int32 [32 * words, >= words] in packed-position order, zeroed by
    the caller (allocated when None); ``coactivation_partner_counts`` applies the map."""
    _dev(zbits, "zbits", torch.int32)
    B, words = zbits.shape
    if zbits.stride(1) != 1:
        zbits = zbits.contiguous()
    index = _packed_index_arg(index, 32 * words)
    partners = _partners_state(partners, 32 * words, zbits.device)
    lib = _lib.load()
    need = int(lib.qsae_coactivation_bits_workspace_bytes(B, 32 * words)) if B > 0 else 0
    ws = _workspace(zbits.device, max(need, 1))
    check(lib.qsae_coactivation_partners_bits(_p(zbits), zbits.stride(0) if B else words, B, 32 * words, _p(index),
                                              _p(partners), partners.stride(0), _p(ws), ws.numel(), _stream()))
    return partners


@_on_tensor_device
def coactivation_partners_sparse(idx: torch.Tensor, val: Optional[torch.Tensor], H: int,
                                 partners: Optional[torch.Tensor] = None) -> torch.Tensor:
    """partners |= "units a and c were active in the same row" from the compact (idx, val) form (active: val > 0; every
    listed entry when val is None; entries outside [0, H) are dropped; a unit listed twice sets its bits once).
    int32 [P, >= P / 32] with P = H rounded up to 32; 1 <= k <= 256."""
    _dev(idx, "idx", torch.int32)
    B, k = idx.shape
    if val is not None:
        _dev(val, "val", torch.float32)
    H = int(H)
    partners = _partners_state(partners, (H + 31) // 32 * 32, idx.device)
    check(_lib.load().qsae_coactivation_partners_sparse(_p(idx.contiguous()),
                                                        _p(val.contiguous()) if val is not None else None, B, k, H,
                                                        _p(partners), partners.stride(0), _stream()))
    return partners


@_on_tensor_device
def coactivation_partner_counts(partners: torch.Tensor, H: int, index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [H]: for every unit, the number of other units that were ever active together with it -- the popcount of
    its row of ``partners`` minus the diagonal bit, in unit order (``index``: packed position -> unit, -1 = none; None =
    identity).  Units without a position get 0."""
    _dev(partners, "partners", torch.int32)
    if partners.dim() != 2 or partners.shape[0] % 32 or partners.shape[1] < partners.shape[0] // 32 or partners.stride(1) != 1:
        raise ValueError("partners: expected an int32 [P, >= P / 32] matrix, P a multiple of 32, with unit column stride")
    P, H = partners.shape[0], int(H)
    index = _packed_index_arg(index, P)
    counts = torch.empty((H,), dtype=torch.int32, device=partners.device)
    check(_lib.load().qsae_coactivation_partner_counts(_p(partners), P, partners.stride(0), _p(index), H, _p(counts),
                                                       _stream()))
    return counts.long()


@_on_tensor_device
def coactivation_partner_counts_dense(coact: torch.Tensor, row0: int = 0) -> torch.Tensor:
    """int64 [R]: counts[i] = #{j != row0 + i : coact[i, j] > 0} for the slab ``coact`` int32 [R, H] of rows row0 ..
    row0 + R - 1 of an [H, H] co-activation matrix (the partner counts of statistics that exist as counts)."""
    _dev(coact, "coact", torch.int32)
    if coact.dim() != 2 or coact.shape[1] == 0:
        raise ValueError("coact: expected an int32 [R, H] matrix")
    if coact.stride(1) != 1:
        coact = coact.contiguous()
    R, H = coact.shape
    counts = torch.empty((R,), dtype=torch.int32, device=coact.device)
    check(_lib.load().qsae_coactivation_partner_counts_dense(_p(coact), coact.stride(0) if R > 1 else H, R, H, int(row0),
                                                             _p(counts), _stream()))
    return counts.long()


def _bitsets(sets: torch.Tensor, size: torch.Tensor, words: int, name: str):
    _dev(sets, f"{name}sets", torch.int32)
    _dev(size, f"{name}size", torch.int32)
    if sets.dim() != 2 or sets.shape[1] < words or size.shape != (sets.shape[0],):
        raise ValueError(f"{name}sets: expected int32 [N, >= {words}] with {name}size int32 [N]")
    if sets.shape[0] and sets.stride(1) != 1:
        sets = sets.contiguous()
    return sets, size.contiguous()


@_on_tensor_device
def token_overlap_hist(asets: torch.Tensor, asize: torch.Tensor, bsets: torch.Tensor, bsize: torch.Tensor, V: int, k: int,
                       hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hist[i, u] += #pairs (a, b) with asize[a] > 0, bsize[b] > 0, |A_a & B_b| = i and asize[a] + bsize[b] - i = u: every
    Jaccard score i / u between the token sets of two SAEs as one table (int64 [k + 1, 2k + 1]), from the packed sets on
    the int8 matrix pipe.  asets / bsets int32 [N, >= ceil(V / 32)]: bit t & 31 of word t >> 5 = token t is in the set
    (a column slice of a wider tensor is read in place; bits at or past V are ignored); asize / bsize int32 [N]: the
    true set sizes, 0 = no set.  1 <= k <= 128.  Pairs whose sizes contradict the bits, or exceed k, are not counted."""
    V, k = int(V), int(k)
    if V <= 0:
        raise ValueError("V must be positive")
    words = (V + 31) // 32
    asets, asize = _bitsets(asets, asize, words, "a")
    bsets, bsize = _bitsets(bsets, bsize, words, "b")
    if hist is None:
        if not 1 <= k <= 128:
            raise ValueError("token_overlap_hist: 1 <= k <= 128 required")
        hist = torch.zeros((k + 1, 2 * k + 1), dtype=torch.int64, device=asets.device)
    else:
        _dev(hist, "hist", torch.int64)
        if hist.shape != (k + 1, 2 * k + 1) or not hist.is_contiguous():
            raise ValueError(f"hist: expected a contiguous int64 [{k + 1}, {2 * k + 1}] tensor")
    Na, Nb = asets.shape[0], bsets.shape[0]
    lib = _lib.load()
    need = int(lib.qsae_token_overlap_hist_workspace_bytes(Na, Nb, V)) if Na and Nb else 0
    ws = _workspace(asets.device, max(need, 1))
    check(lib.qsae_token_overlap_hist(_p(asets), asets.stride(0) if Na else words, _p(asize), Na,
                                      _p(bsets), bsets.stride(0) if Nb else words, _p(bsize), Nb, V, k, _p(hist),
                                      _p(ws), ws.numel(), _stream()))
    return hist


# ---- tokens per feature as ordered CSR lists ---------------------------------------------------------------
def token_lists_workspace_bytes(B: int, H: int) -> int:
    """Bytes of the row bitmap that a token_lists_count* call leaves for token_lists_fill (the formula of
    qsae_token_lists_workspace_bytes, in Python so that a fake registration can size the tensor); 0 for an invalid shape."""
    if B < 0 or H <= 0:
        return 0
    W = max(2, 2 * ((B + 63) // 64))
    return (H * W * 4 + 255) // 256 * 256 + (H * 4 + 255) // 256 * 256


def _token_lists_out(B: int, H: int, device):
    if H <= 0:
        raise ValueError("H must be positive")
    offsets = torch.empty((H + 1,), dtype=torch.int64, device=device)
    # zeroed, not empty: the workspace is an output of the dispatcher op, and its alignment gaps would otherwise differ
    # from call to call; one pass over a bit per (row, unit)
    ws = torch.zeros((token_lists_workspace_bytes(B, H),), dtype=torch.uint8, device=device)
    return offsets, ws


@_on_tensor_device
def token_lists_count(idx: torch.Tensor, val: Optional[torch.Tensor], H: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """First half of a batch's tokens per feature, compact form: -> (offsets int64 [H + 1], workspace uint8).  Row r is
    active in unit idx[r, j] when val[r, j] > 0 (every entry when val is None); offsets[u + 1] - offsets[u] = active rows
    of unit u.  The workspace holds the row bitmap for token_lists_fill.  See qsae_token_lists_count."""
    _dev(idx, "idx", torch.int32)
    if idx.dim() != 2:
        raise ValueError("idx: expected int32 [B, k]")
    B, k = idx.shape
    if val is not None:
        _dev(val, "val", torch.float32)
        if val.shape != idx.shape:
            raise ValueError("val: expected the shape of idx")
        val = val.contiguous()
    idx = idx.contiguous()
    offsets, ws = _token_lists_out(B, int(H), idx.device)
    check(_lib.load().qsae_token_lists_count(_p(idx), _p(val), B, k, int(H), _p(offsets), _p(ws), ws.numel(), _stream()))
    return offsets, ws


@_on_tensor_device
def token_lists_count_bits(zbits: torch.Tensor, H: int, index: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """First half of a batch's tokens per feature, bits form: -> (offsets int64 [H + 1], workspace uint8), offsets in unit
    order.  zbits int32 [B, words] and ``index`` as in coactivation_bits: packed position -> unit, -1 = pad slot (its
    bits are ignored); None = identity (32 * words <= H).  See qsae_token_lists_count_bits."""
    _dev(zbits, "zbits", torch.int32)
    if zbits.dim() != 2:
        raise ValueError("zbits: expected int32 [B, words]")
    B, words = zbits.shape
    if zbits.stride(1) != 1:
        zbits = zbits.contiguous()
    if index is not None:
        if index.dtype not in (torch.int32, torch.int64):
            raise TypeError("index: expected int32 or int64")
        if index.numel() != 32 * words:
            raise ValueError(f"index: expected {32 * words} entries (one per packed position), got {index.numel()}")
        index = _dev(index.to(torch.int32).contiguous(), "index", torch.int32)
    offsets, ws = _token_lists_out(B, int(H), zbits.device)
    check(_lib.load().qsae_token_lists_count_bits(_p(zbits), zbits.stride(0) if B else words, B, 32 * words, _p(index), int(H),
                                                  _p(offsets), _p(ws), ws.numel(), _stream()))
    return offsets, ws


@_on_tensor_device
def token_lists_fill(workspace: torch.Tensor, offsets: torch.Tensor, row_tokens: torch.Tensor, n_entries: int) -> torch.Tensor:
    """Second half: -> tokens int32 [n_entries], tokens[offsets[u] + rank] = row_tokens[r] for every active (r, u) of the
    batch whose count call returned (offsets, workspace); n_entries = int(offsets[-1]).  row_tokens int32 [B]."""
    _dev(workspace, "workspace", torch.uint8)
    _dev(offsets, "offsets", torch.int64)
    _dev(row_tokens, "row_tokens", torch.int32)
    if offsets.dim() != 1 or offsets.numel() < 2 or row_tokens.dim() != 1 or int(n_entries) < 0:
        raise ValueError("token_lists_fill: offsets int64 [H + 1], row_tokens int32 [B] and n_entries >= 0 expected")
    B, H = row_tokens.shape[0], offsets.numel() - 1
    tokens = torch.empty((int(n_entries),), dtype=torch.int32, device=offsets.device)
    check(_lib.load().qsae_token_lists_fill(_p(workspace), workspace.numel(), _p(offsets.contiguous()),
                                            _p(row_tokens.contiguous()), B, H, _p(tokens), int(n_entries), _stream()))
    return tokens


@_on_tensor_device
def token_lists_regroup(batch_offsets: torch.Tensor, segments: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Joins batches: batch_offsets int64 [nb, H + 1] (one row per batch) and segments int32 [nnz] (the batches' tokens
    back to back, in batch order) -> (offsets int64 [H + 1], tokens int32 [nnz]) feature-major, a feature's segments in
    batch order.  See qsae_token_lists_regroup."""
    _dev(batch_offsets, "batch_offsets", torch.int64)
    _dev(segments, "segments", torch.int32)
    if batch_offsets.dim() != 2 or batch_offsets.shape[1] < 2 or segments.dim() != 1:
        raise ValueError("token_lists_regroup: batch_offsets int64 [nb, H + 1] and segments int32 [nnz] expected")
    nb, H = batch_offsets.shape[0], batch_offsets.shape[1] - 1
    batch_offsets, segments = batch_offsets.contiguous(), segments.contiguous()
    offsets = torch.empty((H + 1,), dtype=torch.int64, device=batch_offsets.device)
    tokens = torch.empty_like(segments)
    check(_lib.load().qsae_token_lists_regroup(_p(batch_offsets), nb, H, _p(segments), segments.numel(), _p(offsets),
                                               _p(tokens), _stream()))
    return offsets, tokens


# ---- strongest activations per feature as streaming top-n lists ----------------------------------------------
TOP_EXAMPLES_MAX_N = 64


def _top_examples_keys(keys: torch.Tensor) -> Tuple[int, int]:
    """(H, n) of the state: int64 [H, n] (the bits of the u64 keys), contiguous, on the device, 1 <= n <= 64."""
    _dev(keys, "keys", torch.int64)
    if keys.dim() != 2 or not keys.is_contiguous() or keys.shape[0] < 1 or not 1 <= keys.shape[1] <= TOP_EXAMPLES_MAX_N:
        raise ValueError(f"keys: expected a contiguous int64 [H, n] tensor with 1 <= n <= {TOP_EXAMPLES_MAX_N}, "
                         f"got {tuple(keys.shape)}")
    return keys.shape[0], keys.shape[1]


def _top_examples_base(base: int, B: int) -> int:
    base = int(base)
    if base < 0 or base + B > 2 ** 32:
        raise ValueError(f"top_examples: positions base .. base + B must lie in [0, 2^32], got base = {base}, B = {B}")
    return base


@_on_tensor_device
def top_examples_compact(idx: torch.Tensor, val: Optional[torch.Tensor], floor: float, base: int, keys: torch.Tensor) -> None:
    """keys[h] <- the n largest of keys[h] and this batch's candidates of feature h, in place.  idx int32 [B, k], val fp32
    [B, k] or None (every in-range entry at 1.0); a candidate has val > floor, its position is base + row.  See
    qsae_top_examples_compact."""
    _dev(idx, "idx", torch.int32)
    if idx.dim() != 2:
        raise ValueError("idx: expected int32 [B, k]")
    B, k = idx.shape
    H, n = _top_examples_keys(keys)
    base = _top_examples_base(base, B)
    if val is not None:
        _dev(val, "val", torch.float32)
        if val.shape != idx.shape:
            raise ValueError("val: expected the shape of idx")
        val = val.contiguous()
    idx = idx.contiguous()
    lib = _lib.load()
    need = int(lib.qsae_top_examples_compact_workspace_bytes(B, k, H))
    if need == 0:
        raise ValueError(f"top_examples_compact: B * k = {B * k} is outside what the kernels run (B * k < 2^31)")
    ws = _workspace(idx.device, need)
    check(lib.qsae_top_examples_compact(_p(idx), _p(val), B, k, H, n, float(floor), base, _p(keys), _p(ws), ws.numel(),
                                        _stream()))


@_on_tensor_device
def top_examples_dense(latent: torch.Tensor, floor: float, base: int, keys: torch.Tensor) -> None:
    """The same update from a dense latent fp32 [B, H] (any row stride; a column slice of a wider tensor is read in
    place, and nothing at or past column H is read).  See qsae_top_examples_dense."""
    _dev(latent, "latent", torch.float32)
    H, n = _top_examples_keys(keys)
    if latent.dim() != 2 or latent.shape[1] != H:
        raise ValueError(f"latent: expected fp32 [B, {H}], got {tuple(latent.shape)}")
    B = latent.shape[0]
    base = _top_examples_base(base, B)
    if B and (latent.stride(1) != 1 or latent.stride(0) < H):
        latent = latent.contiguous()
    lib = _lib.load()
    need = int(lib.qsae_top_examples_dense_workspace_bytes(B, H, n))
    ws = _workspace(latent.device, max(need, 16))
    check(lib.qsae_top_examples_dense(_p(latent), latent.stride(0) if B else H, B, H, n, float(floor), base, _p(keys), _p(ws),
                                      ws.numel(), _stream()))


@_on_tensor_device
def top_examples_decode(keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """keys int64 [H, n] -> (values fp32 [H, n], 0.0 for none; positions int64 [H, n], -1 for none; counts int32 [H])."""
    H, n = _top_examples_keys(keys)
    values = torch.empty((H, n), dtype=torch.float32, device=keys.device)
    positions = torch.empty((H, n), dtype=torch.int64, device=keys.device)
    counts = torch.empty((H,), dtype=torch.int32, device=keys.device)
    check(_lib.load().qsae_top_examples_decode(_p(keys), H, n, _p(values), _p(positions), _p(counts), _stream()))
    return values, positions, counts


# ---- evaluation reports: quantization error of a BinarySAE decoder, moments of a dataset --------------------------------
QUANT_ERROR_WORDS = 48          # QSAE_QUANT_ERROR_WORDS: the result block of qsae_quantization_error, 64-bit words
MOMENTS_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


@_on_tensor_device
def quantization_error(logits: torch.Tensor, D: int, n_bits: int, step: float, margin_logit: float):
    """-> (result fp64 [48], unit_err_sq fp64 [H]), both on the device: the statistics of W_quant - W_float of a
    BinarySAE decoder's logits fp32 [H, D * n_bits] in one pass.  The layout of ``result`` (some words are int64 / u64
    bits: ``result.view(torch.int64)``) is the one of qsae_quantization_error in include/qsae.h."""
    logits = _f32c(logits, "logits")
    D, n_bits = int(D), int(n_bits)
    if logits.dim() != 2 or logits.shape[1] != D * n_bits:
        raise ValueError(f"logits is {tuple(logits.shape)}, expected [H, {D * n_bits}]")
    H = logits.shape[0]
    lib = _lib.load()
    result = torch.empty((QUANT_ERROR_WORDS,), dtype=torch.float64, device=logits.device)
    unit_err_sq = torch.empty((H,), dtype=torch.float64, device=logits.device)
    ws = _workspace(logits.device, max(int(lib.qsae_quantization_error_workspace_bytes(H, D, n_bits)), 16))
    check(lib.qsae_quantization_error(_p(logits), H, D, n_bits, float(step), float(margin_logit), _p(result),
                                      _p(unit_err_sq), _p(ws), ws.numel(), _stream()))
    return result, unit_err_sq


@_on_tensor_device
def dataset_moments_add(x: torch.Tensor, recon: Optional[torch.Tensor], group_rows: int, sums: torch.Tensor,
                        counts: torch.Tensor) -> None:
    """sums fp64 [3, D] (per column: sum x, sum x^2, sum (recon - x)^2) and counts int64 [2] (rows kept, rows skipped)
    += the rows of x [B, D] (fp32, fp16 or bf16), in place; groups of ``group_rows`` rows holding a NaN are skipped.
    recon: fp32 [B, D] or None.  See qsae_dataset_moments_add."""
    _dev(x, "x")
    if x.dtype not in MOMENTS_DTYPES:
        raise TypeError(f"x: expected fp32, fp16 or bf16, got {x.dtype}")
    if x.dim() != 2:
        raise ValueError(f"x: expected [B, D], got {tuple(x.shape)}")
    B, D = x.shape
    _dev(sums, "sums", torch.float64)
    _dev(counts, "counts", torch.int64)
    if tuple(sums.shape) != (3, D) or tuple(counts.shape) != (2,) or not sums.is_contiguous() or not counts.is_contiguous():
        raise ValueError(f"state: expected contiguous sums fp64 [3, {D}] and counts int64 [2], got {tuple(sums.shape)} and "
                         f"{tuple(counts.shape)}")
    if sums.device != x.device or counts.device != x.device:
        raise ValueError("x, sums and counts must live on one device")
    if recon is not None:
        recon = _f32c(recon, "recon")
        if recon.shape != x.shape or recon.device != x.device:
            raise ValueError(f"recon: expected the shape and device of x, got {tuple(recon.shape)} on {recon.device}")
    x = x.contiguous()
    group_rows = int(group_rows)
    if group_rows < 1:
        raise ValueError(f"group_rows must be >= 1, got {group_rows}")
    lib = _lib.load()
    ws = _workspace(x.device, max(int(lib.qsae_dataset_moments_workspace_bytes(B, D, group_rows, int(recon is not None))), 16))
    check(lib.qsae_dataset_moments_add(_p(x), MOMENTS_DTYPES[x.dtype], _p(recon), B, D, group_rows, _p(sums), _p(counts),
                                       _p(ws), ws.numel(), _stream()))


@_on_tensor_device
def quantize_bits(x: torch.Tensor, n_bits: int, scale_factor: float, signed: bool = True) -> torch.Tensor:
    """n-bit code of every activation as LSB-first 0/1 floats, [B, D * n_bits] (data/dataset.py:76-102)."""
    x = _f32c(x, "x")
    B, D = x.shape
    out = torch.empty((B, D * n_bits), dtype=torch.float32, device=x.device)
    check(_lib.load().qsae_quantize_bits(_p(x), D, B, D, int(n_bits), float(scale_factor), 1 if signed else 0, _p(out),
                                         _stream()))
    return out


# ---- decoder dictionary comparison -----------------------------------------------------------
def _atoms(t: torch.Tensor, name: str) -> torch.Tensor:
    """fp32 [H, D] rows, contiguous and 16-byte aligned, D padded with zero columns to a multiple of 4 (a zero column
    changes no dot product and no norm)."""
    t = _f32c(t, name)
    if t.dim() != 2:
        raise ValueError(f"{name}: expected [H, D] atoms, got shape {tuple(t.shape)}")
    if t.shape[1] % 4:
        t = torch.nn.functional.pad(t, (0, 4 - t.shape[1] % 4))
    if t.data_ptr() % 16:
        t = t.clone()
    return t


@_on_tensor_device
def atom_inv_norms(atoms: torch.Tensor) -> torch.Tensor:
    """1 / max(||atoms[h]||_2, 1e-12) per row, squares summed in fp64.  fp32 [H]."""
    atoms = _f32c(atoms, "atoms")
    H, D = atoms.shape
    inv = torch.empty((H,), dtype=torch.float32, device=atoms.device)
    check(_lib.load().qsae_atom_inv_norms(_p(atoms), D, H, D, _p(inv), _stream()))
    return inv


COSINE_MAX_THRESHOLDS, COSINE_MAX_BINS = 8, 4096


@_on_tensor_device
def cosine_compare(A: torch.Tensor, B: Optional[torch.Tensor], thresholds=(), bins: int = 0,
                   want_matrix: bool = False):
    """One pass of qsae_cosine_compare over atoms A [Ha, D] and B [Hb, D] (B None: self mode, pairs i < j).
    Returns (row_best int64 [Ha], col_best int64 [Hb] ([0] in self mode), moments fp64 [2], extrema int64 [2],
    counts int64 [len(thresholds)], hist int64 [bins], matrix fp32 [Ha, Hb] or [0, 0]); keys as in include/qsae.h.
    In self mode the matrix is returned whole (the upper triangle mirrored)."""
    self_mode = B is None
    if not self_mode:
        if B.device != A.device:
            raise ValueError(f"A and B are on different devices ({A.device}, {B.device})")
        if B.dim() != 2 or A.dim() != 2 or B.shape[1] != A.shape[1]:
            raise ValueError(f"A and B must be [H, D] atoms of the same D ({tuple(A.shape)}, {tuple(B.shape)})")
    A = _atoms(A, "A")
    Bt = A if self_mode else _atoms(B, "B")
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > COSINE_MAX_THRESHOLDS:
        raise ValueError(f"at most {COSINE_MAX_THRESHOLDS} thresholds")
    if not 0 <= int(bins) <= COSINE_MAX_BINS:
        raise ValueError(f"bins must lie in [0, {COSINE_MAX_BINS}]")
    bins = int(bins)
    Ha, D = A.shape
    Hb = Bt.shape[0]
    if Ha == 0 or Hb == 0:
        raise ValueError("empty dictionary")
    dev = A.device
    i64 = dict(dtype=torch.int64, device=dev)
    row_best = torch.empty((Ha,), **i64)
    col_best = torch.empty((0 if self_mode else Hb,), **i64)
    moments = torch.empty((2,), dtype=torch.float64, device=dev)
    extrema = torch.empty((2,), **i64)
    counts = torch.empty((len(thresholds),), **i64)
    hist = torch.empty((bins,), **i64)
    matrix = torch.empty((Ha, Hb) if want_matrix else (0, 0), dtype=torch.float32, device=dev)
    lib = _lib.load()
    nbytes = lib.qsae_cosine_compare_workspace_bytes(Ha, Hb, 1 if self_mode else 0)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    thr = (C.c_float * max(1, len(thresholds)))(*thresholds)
    check(lib.qsae_cosine_compare(_p(A), D, Ha, None if self_mode else _p(Bt), D, Hb, D, 1 if self_mode else 0,
                                  C.cast(thr, C.c_void_p), len(thresholds), bins, _p(row_best),
                                  None if self_mode else _p(col_best), _p(moments), _p(extrema),
                                  _p(counts) if thresholds else None, _p(hist) if bins else None,
                                  _p(matrix) if want_matrix else None, Hb, _p(ws), nbytes, _stream()))
    if want_matrix and self_mode:
        # the kernel wrote the tiles on and above the diagonal; c(j, i) == c(i, j) bit for bit
        upper = torch.triu(matrix)
        matrix = upper + torch.triu(matrix, 1).t()
    return row_best, col_best, moments, extrema, counts, hist, matrix


# ---- nearest atoms of an int8 dictionary ---------------------------------------------------------------------------
NEAREST_MAX_K, NEAREST_MAX_D = 64, 4096


def _atoms_i8(t: torch.Tensor, name: str) -> torch.Tensor:
    """int8 [N, D] atoms as the kernel reads them: unit inner stride, row stride a multiple of 16 bytes, 16-byte aligned
    (a column slice of a wider aligned tensor is read in place; anything else is copied)."""
    _dev(t, name, torch.int8)
    if t.dim() != 2:
        raise ValueError(f"{name}: expected [N, D] atoms, got shape {tuple(t.shape)}")
    if t.shape[0] and (t.stride(1) != 1 or t.stride(0) % 16 or t.stride(0) < t.shape[1] or t.data_ptr() % 16):
        t = t.contiguous()
        if t.data_ptr() % 16:
            t = t.clone()
    return t


@_on_tensor_device
def nearest_atoms_i8(a: torch.Tensor, b: Optional[torch.Tensor] = None, k: int = 10, exclude_self: bool = False,
                     want_duplicates: bool = False):
    """The k nearest atoms (cosine) of every row of a among the rows of b (None: a itself), int8 [N, D] with D a
    multiple of 32 in [32, 4096], on the int8 matrix pipe (qsae_nearest_atoms_i8; the arithmetic is spelled out in
    include/qsae.h).  Returns (keys int64 [Na, k], duplicate_of int32 [Na] or None): a row's keys descend, 0 = none.
    exclude_self and want_duplicates need self mode."""
    k = int(k)
    self_mode = b is None
    a = _atoms_i8(a, "a")
    if not self_mode:
        if b.device != a.device:
            raise ValueError(f"a and b are on different devices ({a.device}, {b.device})")
        b = _atoms_i8(b, "b")
        if b.shape[1] != a.shape[1]:
            raise ValueError(f"a and b must be [N, D] atoms of the same D ({tuple(a.shape)}, {tuple(b.shape)})")
        if exclude_self or want_duplicates:
            raise ValueError("nearest_atoms_i8: exclude_self / want_duplicates need self mode (b=None)")
    if not 1 <= k <= NEAREST_MAX_K:
        raise ValueError(f"nearest_atoms_i8: 1 <= k <= {NEAREST_MAX_K} required")
    Na, D = a.shape
    if D % 32 or not 32 <= D <= NEAREST_MAX_D:
        raise ValueError(f"nearest_atoms_i8: D must be a multiple of 32 in [32, {NEAREST_MAX_D}] (zero-pad), got {D}")
    Nb = Na if self_mode else b.shape[0]
    keys = torch.empty((Na, k), dtype=torch.int64, device=a.device)
    dup = torch.empty((Na,), dtype=torch.int32, device=a.device) if want_duplicates else None
    lib = _lib.load()
    need = int(lib.qsae_nearest_atoms_i8_workspace_bytes(Na, Nb, D, k)) if Na and Nb else 0
    ws = _workspace(a.device, max(need, 1))
    check(lib.qsae_nearest_atoms_i8(_p(a), a.stride(0) if Na else D, Na, None if self_mode else _p(b),
                                    (b.stride(0) if Nb else D) if not self_mode else 0, Nb, D, k,
                                    1 if exclude_self else 0, _p(keys), _p(dup), _p(ws), ws.numel(), _stream()))
    if Na and not Nb:
        keys.zero_()
    return keys, dup


# ---- nearest atoms of an fp32 dictionary ---------------------------------------------------------------------------
def _atoms_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    """fp32 [N, D] atoms as the kernel reads them: unit inner stride, row stride a multiple of 4 floats, 16-byte aligned
    (a column slice of a wider aligned tensor is read in place; anything else is copied)."""
    _dev(t, name, torch.float32)
    if t.dim() != 2:
        raise ValueError(f"{name}: expected [N, D] atoms, got shape {tuple(t.shape)}")
    if t.shape[0] and (t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < t.shape[1] or t.data_ptr() % 16):
        t = t.contiguous()
        if t.data_ptr() % 16:
            t = t.clone()
    return t


@_on_tensor_device
def nearest_atoms_f32(a: torch.Tensor, b: Optional[torch.Tensor] = None, k: int = 10,
                      exclude_self: bool = False) -> torch.Tensor:
    """The k nearest atoms (cosine) of every row of a among the rows of b (None: a itself), fp32 [N, D] with D a
    multiple of 4, on the exact-fp32 matrix pipe (qsae_nearest_atoms_f32; the arithmetic is spelled out in
    include/qsae.h).  Returns keys int64 [Na, k]: a row's keys descend, 0 = none.  exclude_self needs self mode."""
    k = int(k)
    self_mode = b is None
    a = _atoms_f32(a, "a")
    if not self_mode:
        if b.device != a.device:
            raise ValueError(f"a and b are on different devices ({a.device}, {b.device})")
        b = _atoms_f32(b, "b")
        if b.shape[1] != a.shape[1]:
            raise ValueError(f"a and b must be [N, D] atoms of the same D ({tuple(a.shape)}, {tuple(b.shape)})")
        if exclude_self:
            raise ValueError("nearest_atoms_f32: exclude_self needs self mode (b=None)")
    if not 1 <= k <= NEAREST_MAX_K:
        raise ValueError(f"nearest_atoms_f32: 1 <= k <= {NEAREST_MAX_K} required")
    Na, D = a.shape
    if D <= 0 or D % 4:
        raise ValueError(f"nearest_atoms_f32: D must be a positive multiple of 4 (zero-pad), got {D}")
    Nb = Na if self_mode else b.shape[0]
    keys = torch.empty((Na, k), dtype=torch.int64, device=a.device)
    lib = _lib.load()
    need = int(lib.qsae_nearest_atoms_f32_workspace_bytes(Na, Nb, D, k)) if Na and Nb else 0
    ws = _workspace(a.device, max(need, 1))
    check(lib.qsae_nearest_atoms_f32(_p(a), a.stride(0) if Na else D, Na, None if self_mode else _p(b),
                                     (b.stride(0) if Nb else D) if not self_mode else 0, Nb, D, k,
                                     1 if exclude_self else 0, _p(keys), _p(ws), ws.numel(), _stream()))
    if Na and not Nb:
        keys.zero_()
    return keys


# ---- k-means over dictionary atoms -----------------------------------------------------------------------------------
KMEANS_METRICS = {"cosine": 0, "euclidean": 1}


def _kmeans_pair(atoms: torch.Tensor, centers: torch.Tensor, fn: str):
    atoms = _atoms_f32(atoms, "atoms")
    if not isinstance(centers, torch.Tensor) or centers.device != atoms.device:
        raise ValueError(f"{fn}: atoms and centers are on different devices")
    centers = _atoms_f32(centers, "centers")
    if centers.shape[1] != atoms.shape[1]:
        raise ValueError(f"{fn}: atoms and centers must be [N, D] and [C, D] of the same D ({tuple(atoms.shape)}, "
                         f"{tuple(centers.shape)})")
    D = atoms.shape[1]
    if D <= 0 or D % 4:
        raise ValueError(f"{fn}: D must be a positive multiple of 4 (zero-pad), got {D}")
    if centers.shape[0] < 1:
        raise ValueError(f"{fn}: at least one center required")
    return atoms, centers


@_on_tensor_device
def kmeans_assign(atoms: torch.Tensor, centers: torch.Tensor, metric: str = "cosine") -> torch.Tensor:
    """The assign step of k-means: keys int64 [N], keys[i] = the largest score of atom i over the centers and its center
    (bits of the score << 32 | ~center; equal scores go to the lowest center; 0 = every score was NaN).  fp32 [N, D] and
    [C, D] with D a multiple of 4, on the exact-fp32 matrix pipe (qsae_kmeans_assign_f32; the scores of both metrics are
    spelled out in include/qsae.h).  ``metric``: "cosine" or "euclidean"."""
    if metric not in KMEANS_METRICS:
        raise ValueError(f"kmeans_assign: metric must be 'cosine' or 'euclidean', got {metric!r}")
    atoms, centers = _kmeans_pair(atoms, centers, "kmeans_assign")
    (N, D), Cn = atoms.shape, centers.shape[0]
    keys = torch.empty((N,), dtype=torch.int64, device=atoms.device)
    if N == 0:
        return keys
    lib = _lib.load()
    ws = _workspace(atoms.device, max(int(lib.qsae_kmeans_assign_f32_workspace_bytes(N, Cn, D)), 1))
    check(lib.qsae_kmeans_assign_f32(_p(atoms), atoms.stride(0), N, _p(centers), centers.stride(0), Cn, D,
                                     KMEANS_METRICS[metric], _p(keys), _p(ws), ws.numel(), _stream()))
    return keys


@_on_tensor_device
def kmeans_update(atoms: torch.Tensor, labels: torch.Tensor, centers_old: torch.Tensor):
    """The update step of k-means -> (centers_new fp32 [C, D], counts int32 [C], stats fp64 [2] = {center_shift,
    n_empty}).  ``labels`` [N] (int32 or int64): a label outside [0, C) belongs to no cluster.  A center is the fp64 mean
    of its members in a fixed order (qsae_kmeans_update_f32), rounded once; an empty cluster keeps its old center."""
    atoms, centers_old = _kmeans_pair(atoms, centers_old, "kmeans_update")
    (N, D), Cn = atoms.shape, centers_old.shape[0]
    _dev(labels, "labels")
    if labels.device != atoms.device or labels.shape != (N,) or labels.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"kmeans_update: labels must be int32 or int64 [{N}] on the atoms' device")
    if labels.dtype == torch.int64:                         # out-of-range values stay out of range: no wrap-around
        labels = labels.clamp(-1, Cn).to(torch.int32)
    labels = labels.contiguous()
    if N == 0:
        return (centers_old.clone(), torch.zeros((Cn,), dtype=torch.int32, device=atoms.device),
                torch.tensor([0.0, float(Cn)], dtype=torch.float64, device=atoms.device))
    centers_new = torch.empty((Cn, D), dtype=torch.float32, device=atoms.device)
    counts = torch.empty((Cn,), dtype=torch.int32, device=atoms.device)
    stats = torch.empty((2,), dtype=torch.float64, device=atoms.device)
    lib = _lib.load()
    ws = _workspace(atoms.device, max(int(lib.qsae_kmeans_update_f32_workspace_bytes(N, Cn, D)), 1))
    check(lib.qsae_kmeans_update_f32(_p(atoms), atoms.stride(0), N, D, _p(labels), Cn, _p(centers_old),
                                     centers_old.stride(0), _p(centers_new), D, _p(counts), _p(stats), _p(ws), ws.numel(),
                                     _stream()))
    return centers_new, counts, stats


# ---- BinarySAE training (the gradient of the soft-decoder forward) ---------------------------------------------------
# Workspaces come from the caching allocator per call (not the shared _workspaces cache: a backward may run on another
# thread than the forward).
TRAIN_MAX_D, TRAIN_MAX_K = 4096, 256


def train_supported(D: int, k: int) -> bool:
    return 0 < D <= TRAIN_MAX_D and D % 4 == 0 and 0 <= k <= TRAIN_MAX_K


def _train_ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty((max(1, int(nbytes)),), dtype=torch.uint8, device=device)


@_on_tensor_device
def binary_soft_table_polarize(logits: torch.Tensor, D: int, n_bits: int):
    """-> (soft table fp32 [H, D], polarize fp32 0-d): the table of binary_soft_table and the mean p (1 - p) 2^b that
    BinarySAE.forward reports, both on the device (no host read)."""
    logits = _f32c(logits, "logits")
    H = logits.shape[0]
    if logits.dim() != 2 or logits.shape[1] != D * n_bits:
        raise ValueError(f"logits is {tuple(logits.shape)}, expected [H, {D * n_bits}]")
    table = torch.empty((H, D), dtype=torch.float32, device=logits.device)
    pol = torch.empty((), dtype=torch.float32, device=logits.device)
    lib = _lib.load()
    ws = _train_ws(lib.qsae_binary_soft_table_polarize_workspace_bytes(H, D), logits.device)
    check(lib.qsae_binary_soft_table_polarize(_p(logits), H, D, n_bits, _p(table), _p(pol), _p(ws), ws.numel(), _stream()))
    return table, pol


@_on_tensor_device
def train_csr(idx: torch.Tensor, H: int):
    """Top-k lists [B, k] grouped by unit -> (offsets int32 [H + 1], entries int32 [B k]); see qsae_train_csr."""
    _dev(idx, "idx", torch.int32)
    idx = idx.contiguous()
    B, k = idx.shape
    offsets = torch.empty((H + 1,), dtype=torch.int32, device=idx.device)
    entries = torch.empty((B * k,), dtype=torch.int32, device=idx.device)
    lib = _lib.load()
    ws = _train_ws(lib.qsae_train_csr_workspace_bytes(B, k, H), idx.device)
    check(lib.qsae_train_csr(_p(idx), B, k, H, _p(offsets), _p(entries), _p(ws), ws.numel(), _stream()))
    return offsets, entries


def _check_train_shape(D: int, k: int) -> None:
    if not train_supported(D, k):
        raise ValueError(f"BinarySAE training kernels take D a multiple of 4 up to {TRAIN_MAX_D} and k <= {TRAIN_MAX_K} "
                         f"(got D = {D}, k = {k})")


def _latent_grad(g_latent: Optional[torch.Tensor], B: int, H: int):
    """(tensor, row stride) of an incoming [B, H] latent gradient with unit column stride (autograd may hand in an
    expanded tensor: a stride-0 row broadcast is read as is, anything else is made contiguous)."""
    if g_latent is None:
        return None, 0
    _dev(g_latent, "g_latent")
    if g_latent.dtype != torch.float32:
        g_latent = g_latent.float()
    if tuple(g_latent.shape) != (B, H):
        raise ValueError(f"g_latent is {tuple(g_latent.shape)}, expected [{B}, {H}]")
    if g_latent.stride(1) != 1 or (g_latent.stride(0) != 0 and g_latent.stride(0) < H):
        g_latent = g_latent.contiguous()
    return g_latent, g_latent.stride(0) if B > 1 else H


@_on_tensor_device
def train_row_grad(idx: torch.Tensor, table: torch.Tensor, step: float, g_recon: Optional[torch.Tensor],
                   g_latent: Optional[torch.Tensor], W_enc: Optional[torch.Tensor], want_dx: bool = False):
    """-> (gv fp32 [B, k], dx fp32 [B, D] or None); see qsae_train_row_grad."""
    _dev(idx, "idx", torch.int32)
    idx = idx.contiguous()
    table = _f32c(table, "table")
    B, k = idx.shape
    H, D = table.shape
    _check_train_shape(D, k)
    gR = _f32c(g_recon, "g_recon") if g_recon is not None else None
    if gR is not None and tuple(gR.shape) != (B, D):
        raise ValueError(f"g_recon is {tuple(gR.shape)}, expected [{B}, {D}]")
    gL, gl_ld = _latent_grad(g_latent, B, H)
    W = _f32c(W_enc, "W_enc") if want_dx else None
    if W is not None and tuple(W.shape) != (H, D):
        raise ValueError(f"W_enc is {tuple(W.shape)}, expected [{H}, {D}]")
    gv = torch.empty((B, k), dtype=torch.float32, device=idx.device)
    dx = torch.empty((B, D), dtype=torch.float32, device=idx.device) if want_dx else None
    check(_lib.load().qsae_train_row_grad(_p(idx), B, k, _p(table), H, D, float(step), _p(gR), _p(gL), int(gl_ld),
                                          _p(W), _p(gv), _p(dx), _stream()))
    return gv, dx


@_on_tensor_device
def train_unit_grad(offsets: torch.Tensor, entries: torch.Tensor, val: torch.Tensor, gv: torch.Tensor, x: torch.Tensor,
                    g_recon: Optional[torch.Tensor], logits: torch.Tensor, n_bits: int, step: float,
                    g_polarize: Optional[torch.Tensor], want_encoder: bool = True, want_logits: bool = True):
    """-> (dW_enc [H, D], db_enc [H], dlogits [H, D n_bits]), each None when not wanted; see qsae_train_unit_grad."""
    _dev(offsets, "offsets", torch.int32)
    _dev(entries, "entries", torch.int32)
    val, gv, x, logits = _f32c(val, "val"), _f32c(gv, "gv"), _f32c(x, "x"), _f32c(logits, "logits")
    B, k = val.shape
    D = x.shape[1]
    H = offsets.shape[0] - 1
    _check_train_shape(D, k)
    if tuple(logits.shape) != (H, D * n_bits) or tuple(x.shape) != (B, D) or tuple(gv.shape) != (B, k) \
            or entries.numel() != B * k:
        raise ValueError("train_unit_grad: inconsistent shapes")
    gR = _f32c(g_recon, "g_recon") if g_recon is not None else None
    if gR is not None and tuple(gR.shape) != (B, D):
        raise ValueError(f"g_recon is {tuple(gR.shape)}, expected [{B}, {D}]")
    gP = _f32c(g_polarize.reshape(()), "g_polarize") if g_polarize is not None else None
    dev = x.device
    dW = torch.empty((H, D), dtype=torch.float32, device=dev) if want_encoder else None
    db = torch.empty((H,), dtype=torch.float32, device=dev) if want_encoder else None
    dl = torch.empty((H, D * n_bits), dtype=torch.float32, device=dev) if want_logits else None
    lib = _lib.load()
    ws = _train_ws(lib.qsae_train_unit_grad_workspace_bytes(B, k, H, D), dev)
    check(lib.qsae_train_unit_grad(_p(offsets.contiguous()), _p(entries.contiguous()), _p(val), _p(gv), B, k, _p(x), _p(gR),
                                   _p(logits), H, D, n_bits, float(step), _p(gP), _p(dW), _p(db), _p(dl), _p(ws),
                                   ws.numel(), _stream()))
    return dW, db, dl


@_on_tensor_device
def train_col_sum(g: torch.Tensor) -> torch.Tensor:
    """sum over rows of g [B, D] in a fixed order (the decoder-bias gradient)."""
    g = _f32c(g, "g")
    B, D = g.shape
    out = torch.empty((D,), dtype=torch.float32, device=g.device)
    lib = _lib.load()
    ws = _train_ws(lib.qsae_train_col_sum_workspace_bytes(B, D), g.device)
    check(lib.qsae_train_col_sum(_p(g), B, D, _p(out), _p(ws), ws.numel(), _stream()))
    return out


# ---- BaselineSparseAutoencoder training ---------------------------------------------------------------------------------
@_on_tensor_device
def train_table_unit_grad(offsets: torch.Tensor, entries: torch.Tensor, val: torch.Tensor, gv: torch.Tensor, x: torch.Tensor,
                          g_recon: Optional[torch.Tensor], want_encoder: bool = True, want_decoder: bool = True):
    """-> (dW_enc [H, D], db_enc [H], dW_dec [D, H] in the layout of nn.Linear(H, D).weight), each None when not wanted;
    see qsae_train_table_unit_grad."""
    _dev(offsets, "offsets", torch.int32)
    _dev(entries, "entries", torch.int32)
    val, gv, x = _f32c(val, "val"), _f32c(gv, "gv"), _f32c(x, "x")
    if val.dim() != 2 or x.dim() != 2 or offsets.dim() != 1:
        raise ValueError("train_table_unit_grad: val and x must be 2-D, offsets 1-D")
    B, k = val.shape
    D = x.shape[1]
    H = offsets.shape[0] - 1
    _check_train_shape(D, k)
    if H < 1 or tuple(x.shape) != (B, D) or tuple(gv.shape) != (B, k) or entries.numel() != B * k:
        raise ValueError("train_table_unit_grad: inconsistent shapes")
    if B * k >= 2 ** 31:
        raise ValueError(f"train_table_unit_grad: B * k = {B * k} is not below 2^31")
    gR = _f32c(g_recon, "g_recon") if g_recon is not None else None
    if gR is not None and tuple(gR.shape) != (B, D):
        raise ValueError(f"g_recon is {tuple(gR.shape)}, expected [{B}, {D}]")
    dev = x.device
    dW = torch.empty((H, D), dtype=torch.float32, device=dev) if want_encoder else None
    db = torch.empty((H,), dtype=torch.float32, device=dev) if want_encoder else None
    dWd = torch.empty((D, H), dtype=torch.float32, device=dev) if want_decoder else None
    lib = _lib.load()
    ws = _train_ws(lib.qsae_train_table_unit_grad_workspace_bytes(B, k, H, D), dev)
    check(lib.qsae_train_table_unit_grad(_p(offsets.contiguous()), _p(entries.contiguous()), _p(val), _p(gv), B, k, _p(x),
                                         _p(gR), H, D, _p(dW), _p(db), _p(dWd), H, _p(ws), ws.numel(), _stream()))
    return dW, db, dWd


def normalize_columns_supported(H: int) -> bool:
    return H > 0 and H % 4 == 0


@_on_tensor_device
def normalize_columns_table(W: torch.Tensor, want_table: bool = True) -> Optional[torch.Tensor]:
    """Unit-norm columns of W [D, H] IN PLACE (W / clamp(norm(W, dim=0), min=1e-8)); -> the normalised transpose [H, D]
    (None unless want_table); see qsae_normalize_columns_table."""
    _dev(W, "W", torch.float32)
    if W.dim() != 2 or W.shape[0] < 1 or not normalize_columns_supported(W.shape[1]):
        raise ValueError(f"normalize_columns_table: W is {tuple(W.shape)}, expected [D >= 1, H a multiple of 4]")
    if not W.is_contiguous() or W.data_ptr() % 16 != 0:
        raise ValueError("normalize_columns_table: W must be contiguous and 16-byte aligned (it is updated in place)")
    D, H = W.shape
    table = torch.empty((H, D), dtype=torch.float32, device=W.device) if want_table else None
    check(_lib.load().qsae_normalize_columns_table(_p(W), D, H, _p(table), _stream()))
    return table


# ---- QuantizedMatryoshkaSAE training -------------------------------------------------------------------------------------
def train_matryoshka_supported(D: int) -> bool:
    return 0 < D <= TRAIN_MAX_D and D % 4 == 0


def _check_matryoshka_shape(D: int) -> None:
    if not train_matryoshka_supported(D):
        raise ValueError(f"QuantizedMatryoshkaSAE training kernels take D a multiple of 4 up to {TRAIN_MAX_D} (got D = {D})")


def _i32dev(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    _dev(t, name)
    return t.to(torch.int32).contiguous()


@_on_tensor_device
def transpose_rows(src: torch.Tensor) -> torch.Tensor:
    """[H, D] fp32 -> its transpose [D, H] as a contiguous copy (D a multiple of 4); see qsae_transpose_rows."""
    src = _f32c(src, "src")
    H, D = src.shape
    dst = torch.empty((D, H), dtype=torch.float32, device=src.device)
    check(_lib.load().qsae_transpose_rows(_p(src), H, D, _p(dst), _stream()))
    return dst


@_on_tensor_device
def train_pre_bits(pre: torch.Tensor) -> torch.Tensor:
    """int32-packed z bits [B, H / 32] of a pre-activation [B, H] (H a multiple of 32) by the cutoff every bits path uses;
    see qsae_train_pre_bits."""
    _dev(pre, "pre", torch.float32)
    if pre.dim() != 2 or not pre.is_contiguous() or pre.shape[1] % 32:
        raise ValueError(f"train_pre_bits: pre must be a contiguous [B, H] tensor with H a multiple of 32, got {tuple(pre.shape)}")
    B, H = pre.shape
    z = torch.empty((B, H // 32), dtype=torch.int32, device=pre.device)
    check(_lib.load().qsae_train_pre_bits(_p(pre), H, B, H, _p(z), H // 32, _stream()))
    return z


@_on_tensor_device
def train_matryoshka_sign_rows(w: torch.Tensor, wm: torch.Tensor, index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> S fp32 [slots, D] in {-2, 0, 2} in the packed hidden order (index int32 [slots] or None = the parameters' order)."""
    w, wm = _f32c(w, "w"), _f32c(wm, "wm")
    D = w.shape[1]
    _check_matryoshka_shape(D)
    index = _i32dev(index, "index")
    slots = index.numel() if index is not None else w.shape[0]
    S = torch.empty((slots, D), dtype=torch.float32, device=w.device)
    check(_lib.load().qsae_train_matryoshka_sign_rows(_p(w), _p(wm), _p(index), slots, D, _p(S), _stream()))
    return S


def _levels_grad(g_levels: Optional[torch.Tensor], n_bits: int, B: int, D: int):
    if g_levels is None:
        return None
    g = _f32c(g_levels, "g_levels")
    if tuple(g.shape) != (n_bits, B, D):
        raise ValueError(f"g_levels is {tuple(g.shape)}, expected [{n_bits}, {B}, {D}]")
    return g


@_on_tensor_device
def train_matryoshka_dpre(pre: torch.Tensor, g_levels: Optional[torch.Tensor], g_groups: Optional[torch.Tensor],
                          sign_rows: torch.Tensor, scale: torch.Tensor, sizes) -> torch.Tensor:
    """The pre-activation [B, H] (contiguous fp32, packed hidden order) becomes dpre IN PLACE and is returned; see
    qsae_train_matryoshka_dpre."""
    _dev(pre, "pre", torch.float32)
    if pre.dim() != 2 or not pre.is_contiguous():
        raise ValueError("train_matryoshka_dpre: pre must be a contiguous [B, H] tensor (it is updated in place)")
    _latent_pool_forget(pre)
    B, H = pre.shape
    sign_rows, scale = _f32c(sign_rows, "sign_rows"), _f32c(scale, "scale")
    D = sign_rows.shape[1]
    _check_matryoshka_shape(D)
    n_bits = len(sizes)
    if sign_rows.shape[0] != H or scale.numel() != H or sum(sizes) != H or B < 1:
        raise ValueError("train_matryoshka_dpre: inconsistent shapes")
    G = _levels_grad(g_levels, n_bits, B, D)
    gg = _f32c(g_groups.reshape(-1), "g_groups") if g_groups is not None else None
    if gg is not None and gg.numel() != n_bits:
        raise ValueError(f"g_groups has {gg.numel()} elements, expected {n_bits}")
    keep, sp = _sizes_arg(sizes, n_bits)
    check(_lib.load().qsae_train_matryoshka_dpre(_p(G), _p(gg), _p(sign_rows), _p(scale), B, D, H, n_bits, sp, _p(pre), H,
                                                 _stream()))
    return pre


@_on_tensor_device
def train_gemm_tn(A: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """A [K, M], X [K, N] -> A^T X [M, N] as one fp32 chain per element in ascending k; see qsae_train_gemm_tn."""
    A, X = _f32c(A, "A"), _f32c(X, "X")
    K, M = A.shape
    N = X.shape[1]
    if X.shape[0] != K or K < 1 or M % 4 or N % 4:
        raise ValueError(f"train_gemm_tn: A {tuple(A.shape)}, X {tuple(X.shape)}: equal K >= 1, M and N multiples of 4")
    out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    check(_lib.load().qsae_train_gemm_tn(_p(A), M, _p(X), N, K, M, N, _p(out), N, _stream()))
    return out


@_on_tensor_device
def train_matryoshka_dsum_dense(zbits: torch.Tensor, g_levels: torch.Tensor, H: int, sizes) -> torch.Tensor:
    """-> dSum fp32 [H, D] from the z bits and the incoming gradients [n, B, D]; see qsae_train_matryoshka_dsum_dense."""
    _dev(zbits, "zbits", torch.int32)
    B = zbits.shape[0]
    n_bits = len(sizes)
    D = g_levels.shape[2]
    _check_matryoshka_shape(D)
    G = _levels_grad(g_levels, n_bits, B, D)
    if zbits.stride(1) != 1 or zbits.shape[1] * 32 < H or sum(sizes) != H or B < 1:
        raise ValueError("train_matryoshka_dsum_dense: inconsistent shapes")
    dsum = torch.empty((H, D), dtype=torch.float32, device=zbits.device)
    keep, sp = _sizes_arg(sizes, n_bits)
    check(_lib.load().qsae_train_matryoshka_dsum_dense(_p(zbits), zbits.stride(0), _p(G), B, D, H, n_bits, sp, _p(dsum),
                                                       _stream()))
    return dsum


def train_bits_csr_supported(B: int, H: int) -> bool:
    return B >= 1 and H > 0 and H % 32 == 0 and B * H < 2 ** 31


@_on_tensor_device
def train_bits_csr(zbits: torch.Tensor, H: int, n_entries: int):
    """z bits [B, words] -> (offsets int32 [H + 1], entries int32 [n_entries]): the active rows of every unit, ascending;
    n_entries is the batch's active-unit count (the decoder's level counts).  See qsae_train_bits_csr."""
    _dev(zbits, "zbits", torch.int32)
    B = zbits.shape[0]
    if not train_bits_csr_supported(B, H) or zbits.stride(1) != 1 or zbits.shape[1] * 32 < H:
        raise ValueError(f"train_bits_csr: the unit lists take H a multiple of 32 and B * H < 2^31 (got B = {B}, H = {H})")
    offsets = torch.empty((H + 1,), dtype=torch.int32, device=zbits.device)
    entries = torch.empty((max(1, int(n_entries)),), dtype=torch.int32, device=zbits.device)
    lib = _lib.load()
    ws = _train_ws(lib.qsae_train_bits_csr_workspace_bytes(B, H), zbits.device)
    check(lib.qsae_train_bits_csr(_p(zbits), zbits.stride(0), B, H, _p(offsets), _p(entries), int(n_entries), _p(ws),
                                  ws.numel(), _stream()))
    return offsets, entries


@_on_tensor_device
def train_matryoshka_dsum_lists(offsets: torch.Tensor, entries: torch.Tensor, n_entries: int, g_levels: torch.Tensor,
                                sizes) -> torch.Tensor:
    """-> dSum fp32 [H, D] summed over the unit lists of train_bits_csr; see qsae_train_matryoshka_dsum_lists."""
    _dev(offsets, "offsets", torch.int32)
    _dev(entries, "entries", torch.int32)
    n_bits, B, D = g_levels.shape
    _check_matryoshka_shape(D)
    H = offsets.shape[0] - 1
    if len(sizes) != n_bits or sum(sizes) != H or B < 1 or not 0 <= n_entries < 2 ** 31:
        raise ValueError("train_matryoshka_dsum_lists: inconsistent shapes")
    G = _levels_grad(g_levels, n_bits, B, D)
    dsum = torch.empty((H, D), dtype=torch.float32, device=G.device)
    lib = _lib.load()
    ws = _train_ws(lib.qsae_train_matryoshka_dsum_lists_workspace_bytes(B, int(n_entries), H, D), G.device)
    keep, sp = _sizes_arg(sizes, n_bits)
    check(lib.qsae_train_matryoshka_dsum_lists(_p(offsets.contiguous()), _p(entries.contiguous()), int(n_entries), _p(G), B, D,
                                               H, n_bits, sp, _p(dsum), _p(ws), ws.numel(), _stream()))
    return dsum


@_on_tensor_device
def train_matryoshka_finish(dsum: Optional[torch.Tensor], scale: torch.Tensor, index: Optional[torch.Tensor],
                            w: torch.Tensor, wm: torch.Tensor):
    """-> (dweight, dweight_mirror) [H, D] in the parameters' order; see qsae_train_matryoshka_finish."""
    w, wm, scale = _f32c(w, "w"), _f32c(wm, "wm"), _f32c(scale, "scale")
    D = w.shape[1]
    _check_matryoshka_shape(D)
    slots = scale.numel()
    index = _i32dev(index, "index")
    if (index is None and slots != w.shape[0]) or (index is not None and index.numel() != slots) or w.shape != wm.shape:
        raise ValueError("train_matryoshka_finish: inconsistent shapes")
    ds = _f32c(dsum, "dsum") if dsum is not None else None
    if ds is not None and tuple(ds.shape) != (slots, D):
        raise ValueError(f"dsum is {tuple(ds.shape)}, expected [{slots}, {D}]")
    dw, dwm = torch.empty_like(w), torch.empty_like(wm)
    check(_lib.load().qsae_train_matryoshka_finish(_p(ds), _p(scale), _p(index), _p(w), _p(wm), slots, D, _p(dw), _p(dwm),
                                                   _stream()))
    return dw, dwm


@_on_tensor_device
def train_matryoshka_secant(gw: torch.Tensor, gwm: torch.Tensor, counts: torch.Tensor, c: float, scale: torch.Tensor,
                            index: Optional[torch.Tensor], w: torch.Tensor, wm: torch.Tensor) -> None:
    """The secant correction of apply_secant_grad() on the two gradient tensors IN PLACE; see qsae_train_matryoshka_secant."""
    for t, name in ((gw, "weight.grad"), (gwm, "weight_mirror.grad")):
        _dev(t, name, torch.float32)
        if not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"train_matryoshka_secant: {name} must be contiguous and 16-byte aligned (it is updated in place)")
    w, wm, scale = _f32c(w, "w"), _f32c(wm, "wm"), _f32c(scale, "scale")
    _dev(counts, "counts", torch.int64)
    D = w.shape[1]
    _check_matryoshka_shape(D)
    slots = scale.numel()
    index = _i32dev(index, "index")
    if counts.numel() < slots or gw.shape != w.shape or gwm.shape != wm.shape or \
            (index is None and slots != w.shape[0]) or (index is not None and index.numel() != slots):
        raise ValueError("train_matryoshka_secant: inconsistent shapes")
    check(_lib.load().qsae_train_matryoshka_secant(_p(counts.contiguous()), float(c), _p(scale), _p(index), _p(w), _p(wm),
                                                   slots, D, _p(gw), _p(gwm), _stream()))


# ---- TernarySparseAutoencoder training -------------------------------------------------------------------------------------
def train_ternary_supported(D: int, H: int) -> bool:
    return 0 < D <= TRAIN_MAX_D and D % 4 == 0 and H > 0 and H % 4 == 0


def train_mask_supported(D: int, H: int) -> bool:
    return D > 0 and H > 0 and D * H < 2 ** 31 and (D * H) % 4 == 0


@_on_tensor_device
def train_ternary_rows(w: torch.Tensor) -> torch.Tensor:
    """decoder.weight [D, H] -> the fp32 ternary dictionary transposed, [H, D] in {-1, 0, +1}; see qsae_train_ternary_rows."""
    w = _f32c(w, "w")
    D, H = w.shape
    if H % 4:
        raise ValueError(f"train_ternary_rows: hidden_dim must be a multiple of 4 (got {H})")
    out = torch.empty((H, D), dtype=torch.float32, device=w.device)
    check(_lib.load().qsae_train_ternary_rows(_p(w), D, H, _p(out), _stream()))
    return out


@_on_tensor_device
def train_ternary_dpre(h: torch.Tensor, g_recon: Optional[torch.Tensor], g_latent: Optional[torch.Tensor],
                       t_rows: torch.Tensor) -> torch.Tensor:
    """-> dpre [B, H] (a new tensor; h is only read); see qsae_train_ternary_dpre."""
    h, t_rows = _f32c(h, "h"), _f32c(t_rows, "t_rows")
    B, H = h.shape
    D = t_rows.shape[1]
    if not train_ternary_supported(D, H) or t_rows.shape[0] != H or B < 1:
        raise ValueError(f"train_ternary_dpre: D a multiple of 4 up to {TRAIN_MAX_D}, H a multiple of 4 (got D = {D}, H = {H})")
    G = _f32c(g_recon, "g_recon") if g_recon is not None else None
    gh = _f32c(g_latent, "g_latent") if g_latent is not None else None
    if (G is not None and tuple(G.shape) != (B, D)) or (gh is not None and tuple(gh.shape) != (B, H)):
        raise ValueError("train_ternary_dpre: inconsistent shapes")
    dpre = torch.empty_like(h)
    check(_lib.load().qsae_train_ternary_dpre(_p(G), _p(t_rows), _p(gh), _p(h), B, D, H, _p(dpre), _stream()))
    return dpre


@_on_tensor_device
def train_ternary_dweight(g_recon: torch.Tensor, h: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """-> mask * (g_recon^T h) [D, H]; see qsae_train_ternary_dweight."""
    G, h, mask = _f32c(g_recon, "g_recon"), _f32c(h, "h"), _f32c(mask, "mask")
    B, D = G.shape
    H = h.shape[1]
    if not train_ternary_supported(D, H) or h.shape[0] != B or tuple(mask.shape) != (D, H) or B < 1:
        raise ValueError(f"train_ternary_dweight: D a multiple of 4 up to {TRAIN_MAX_D}, H a multiple of 4 (got D = {D}, H = {H})")
    out = torch.empty((D, H), dtype=torch.float32, device=G.device)
    check(_lib.load().qsae_train_ternary_dweight(_p(G), _p(h), _p(mask), B, D, H, _p(out), _stream()))
    return out


# ---- BinaryLatentSAE training -------------------------------------------------------------------------------------------
def train_blatent_supported(D: int, H: int) -> bool:
    return 0 < D <= TRAIN_MAX_D and D % 4 == 0 and H > 0 and H % 32 == 0


_BLATENT_LIMITS = f"D a multiple of 4 up to {TRAIN_MAX_D}, H a multiple of 32, B >= 1 and B * H below 2^31"


@_on_tensor_device
def blatent_binarize(pre: torch.Tensor, cutoff: float, want_latent: bool = True):
    """pre [B, H] -> (latent fp32 [B, H] = (pre >= cutoff) or None, zbits int32 [B, H / 32]) in one pass; see
    qsae_blatent_binarize."""
    _dev(pre, "pre", torch.float32)
    if pre.dim() != 2 or not pre.is_contiguous() or pre.shape[0] < 1 or pre.shape[1] < 1 or pre.shape[1] % 32 \
            or pre.numel() >= 2 ** 31:
        raise ValueError(f"blatent_binarize: pre must be a contiguous [B, H] tensor with H a multiple of 32, B >= 1 and "
                         f"B * H below 2^31, got {tuple(pre.shape)}")
    B, H = pre.shape
    latent = torch.empty_like(pre) if want_latent else None
    zbits = torch.empty((B, H // 32), dtype=torch.int32, device=pre.device)
    check(_lib.load().qsae_blatent_binarize(_p(pre), B, H, float(cutoff), _p(latent), _p(zbits), _stream()))
    return latent, zbits


@_on_tensor_device
def train_blatent_dpre(pre: torch.Tensor, g_recon: torch.Tensor, w_dec: torch.Tensor) -> torch.Tensor:
    """The pre-activation [B, H] (contiguous fp32) becomes dpre IN PLACE and is returned; w_dec is decoder.weight [D, H] as it
    lies; see qsae_train_blatent_dpre."""
    _dev(pre, "pre", torch.float32)
    if pre.dim() != 2 or not pre.is_contiguous():
        raise ValueError("train_blatent_dpre: pre must be a contiguous [B, H] tensor (it is updated in place)")
    _latent_pool_forget(pre)
    B, H = pre.shape
    G, w_dec = _f32c(g_recon, "g_recon"), _f32c(w_dec, "w_dec")
    D = w_dec.shape[0]
    if not train_blatent_supported(D, H) or B < 1 or B * H >= 2 ** 31:
        raise ValueError(f"train_blatent_dpre: {_BLATENT_LIMITS} (got B = {B}, D = {D}, H = {H})")
    if tuple(w_dec.shape) != (D, H) or tuple(G.shape) != (B, D):
        raise ValueError("train_blatent_dpre: inconsistent shapes")
    check(_lib.load().qsae_train_blatent_dpre(_p(G), _p(w_dec), B, D, H, _p(pre), _stream()))
    return pre


@_on_tensor_device
def train_blatent_dweight(g_recon: torch.Tensor, zbits: torch.Tensor, H: int) -> torch.Tensor:
    """-> g_recon^T z [D, H] in the layout of decoder.weight, z expanded from zbits [B, H / 32]; see
    qsae_train_blatent_dweight."""
    _dev(zbits, "zbits", torch.int32)
    G = _f32c(g_recon, "g_recon")
    B, D = G.shape
    if not train_blatent_supported(D, H) or B < 1 or B * H >= 2 ** 31:
        raise ValueError(f"train_blatent_dweight: {_BLATENT_LIMITS} (got B = {B}, D = {D}, H = {H})")
    if zbits.dim() != 2 or zbits.shape[0] != B or zbits.stride(1) != 1 or zbits.shape[1] * 32 < H:
        raise ValueError("train_blatent_dweight: inconsistent shapes")
    out = torch.empty((D, H), dtype=torch.float32, device=G.device)
    check(_lib.load().qsae_train_blatent_dweight(_p(G), _p(zbits), zbits.stride(0), B, D, H, _p(out), _stream()))
    return out


def _mask_operands(w: torch.Tensor, mask: torch.Tensor, what: str):
    for t, name in ((w, "weight"), (mask, "mask")):
        _dev(t, name, torch.float32)
        if t.dim() != 2 or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"{what}: {name} must be a contiguous, 16-byte aligned [D, H] tensor (it is updated in place)")
    D, H = w.shape
    if tuple(mask.shape) != (D, H):
        raise ValueError(f"{what}: mask is {tuple(mask.shape)}, weight {tuple(w.shape)}")
    if not train_mask_supported(D, H):
        raise ValueError(f"{what}: the mask kernels take D * H below 2^31 and a multiple of 4 (got D = {D}, H = {H})")
    return D, H


@_on_tensor_device
def train_mask_init(w: torch.Tensor, mask: torch.Tensor, n_inactive: int) -> None:
    """init_mask on weight / mask [D, H] IN PLACE; see qsae_train_mask_init."""
    D, H = _mask_operands(w, mask, "train_mask_init")
    if not 0 <= n_inactive <= D * H:
        raise ValueError(f"train_mask_init: {n_inactive} inactive positions of {D * H}")
    lib = _lib.load()
    ws = _train_ws(lib.qsae_train_mask_workspace_bytes(D, H), w.device)
    check(lib.qsae_train_mask_init(_p(w), _p(mask), D, H, int(n_inactive), _p(ws), ws.numel(), _stream()))


@_on_tensor_device
def train_mask_update(w: torch.Tensor, mask: torch.Tensor, a: Optional[torch.Tensor], delta: Optional[torch.Tensor],
                      n: int) -> None:
    """update_mask on weight / mask [D, H] IN PLACE (a [H], delta [D], or both None: drop only); see qsae_train_mask_update."""
    D, H = _mask_operands(w, mask, "train_mask_update")
    if not 0 <= n <= D * H:
        raise ValueError(f"train_mask_update: n = {n} is outside 0 .. {D * H}")
    if (a is None) != (delta is None):
        raise ValueError("train_mask_update: a and delta are given together or not at all")
    if a is not None:
        a, delta = _f32c(a, "a"), _f32c(delta, "delta")
        if a.numel() != H or delta.numel() != D:
            raise ValueError(f"train_mask_update: a has {a.numel()} elements (H = {H}), delta {delta.numel()} (D = {D})")
    lib = _lib.load()
    ws = _train_ws(lib.qsae_train_mask_workspace_bytes(D, H), w.device)
    check(lib.qsae_train_mask_update(_p(w), _p(mask), _p(a), _p(delta), D, H, int(n), _p(ws), ws.numel(), _stream()))


# ---- optimizer: the Adam step (csrc/optim.hip; quantizedsae_amd.optim.Adam is the user) -----------------------------------------
def _adam_operands(who: str, names, tensors) -> None:
    first = tensors[0]
    for name, t in zip(names, tensors):
        _dev(t, f"{who}: {name}", torch.float32)
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous (p, m and v are updated in place)")
        if t.shape != first.shape or t.device != first.device:
            raise ValueError(f"{who}: {name} is {tuple(t.shape)} on {t.device}, {names[0]} is {tuple(first.shape)} "
                             f"on {first.device}")


@_on_tensor_device
def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, one_minus_b1: float, b2: float,
              one_minus_b2: float, bc2_sqrt: float, eps: float, step_size: float) -> None:
    """One Adam step on p, m, v IN PLACE from the gradient g (all fp32, contiguous, the same shape; a view that starts off a
    16-byte boundary is fine).  The scalars are Python floats, each rounded to fp32 once here; see qsae_adam_step."""
    _adam_operands("adam_step", ("p", "g", "m", "v"), (p, g, m, v))
    check(_lib.load().qsae_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps,
                                     step_size, _stream()))


@_on_tensor_device
def adam_step_prefilter(W: torch.Tensor, gW: torch.Tensor, mW: torch.Tensor, vW: torch.Tensor,
                        bias: Optional[torch.Tensor], gb: Optional[torch.Tensor], mb: Optional[torch.Tensor],
                        vb: Optional[torch.Tensor], one_minus_b1: float, b2: float, one_minus_b2: float, bc2_sqrt: float,
                        eps: float, step_size: float, Wq: Optional[torch.Tensor] = None,
                        meta: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """adam_step on the encoder weight W [H, D] and (all four given, or all four None) its bias [H], IN PLACE; -> (Wq, meta),
    bit-identical to prefilter_pack_w(W, bias) of the updated values.  ``Wq`` (fp16 [H, D]) / ``meta`` (fp32 [4]): buffers
    to write into instead of new ones.  See qsae_adam_step_prefilter."""
    who = "adam_step_prefilter"
    _adam_operands(who, ("W", "gW", "mW", "vW"), (W, gW, mW, vW))
    if W.dim() != 2 or W.numel() == 0:
        raise ValueError(f"{who}: W is {tuple(W.shape)}, expected [H >= 1, D >= 1]")
    H, D = W.shape
    quad = (bias, gb, mb, vb)
    if any(t is None for t in quad) and not all(t is None for t in quad):
        raise ValueError(f"{who}: bias, gb, mb and vb are given together or not at all")
    if bias is not None:
        _adam_operands(who, ("bias", "gb", "mb", "vb"), quad)
        if tuple(bias.shape) != (H,) or bias.device != W.device:
            raise ValueError(f"{who}: bias is {tuple(bias.shape)} on {bias.device}, W is {tuple(W.shape)} on {W.device}")
    if W.data_ptr() % 16 != 0:
        raise ValueError(f"{who}: W must be 16-byte aligned (the prefilter entry points ask for that too)")
    if Wq is None:
        Wq = torch.empty((H, D), dtype=torch.float16, device=W.device)
    if meta is None:
        meta = torch.empty((4,), dtype=torch.float32, device=W.device)
    _dev(Wq, f"{who}: Wq", torch.float16)
    _dev(meta, f"{who}: meta", torch.float32)
    if tuple(Wq.shape) != (H, D) or tuple(meta.shape) != (4,) or not Wq.is_contiguous() or not meta.is_contiguous() \
            or Wq.device != W.device or meta.device != W.device or Wq.data_ptr() % 16 != 0:
        raise ValueError(f"{who}: Wq must be a contiguous 16-byte aligned fp16 [{H}, {D}] and meta a contiguous fp32 [4] on "
                         f"{W.device}")
    check(_lib.load().qsae_adam_step_prefilter(_p(W), _p(gW), _p(mW), _p(vW), _p(bias), _p(gb), _p(mb), _p(vb), H, D,
                                               one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size, _p(Wq), _p(meta),
                                               _stream()))
    return Wq, meta


# ---- the recipe around the step (csrc/optim_recipe.hip, include/qsae_optim.h; quantizedsae_amd.optim.Adam is the user) ----------
GRAD_NORM_HEAD = 4
GRAD_NORM_MAX_TENSORS = 65536


def project_columns_supported(H: int) -> bool:
    """qsaeo_project_columns takes H a multiple of 4 (the limit of normalize_columns_table)"""
    return H > 0 and H % 4 == 0


@_on_tensor_device
def project_columns(W: torch.Tensor, G: torch.Tensor) -> None:
    """G [D, H] (the gradient of W, updated IN PLACE) loses, column by column, its component along the column of W [D, H]:
    G[:, h] -= (G[:, h] . W[:, h]) * W[:, h].  Both fp32, 16-byte aligned, rows contiguous with the same row stride (a
    multiple of 4 elements).  See qsaeo_project_columns for the order of the sums."""
    who = "project_columns"
    _dev(W, f"{who}: W", torch.float32)
    _dev(G, f"{who}: G", torch.float32)
    if W.dim() != 2 or G.shape != W.shape or G.device != W.device:
        raise ValueError(f"{who}: W is {tuple(W.shape)} on {W.device}, G is {tuple(G.shape)} on {G.device}; expected two [D, H]")
    D, H = W.shape
    if D == 0 or H == 0:
        return
    if not project_columns_supported(H):
        raise ValueError(f"{who}: W is {tuple(W.shape)}, expected [D >= 1, H a multiple of 4]")
    ld = W.stride(0) if D > 1 else max(H, W.stride(0))
    if W.stride(1) != 1 or G.stride(1) != 1 or (D > 1 and G.stride(0) != ld) or ld < H or ld % 4 != 0:
        raise ValueError(f"{who}: W and G must have unit inner stride and the same row stride, a multiple of 4 (strides "
                         f"{W.stride()} and {G.stride()})")
    if W.data_ptr() % 16 != 0 or G.data_ptr() % 16 != 0:
        raise ValueError(f"{who}: W and G must be 16-byte aligned")
    if W.data_ptr() == G.data_ptr():
        raise ValueError(f"{who}: W and G are the same memory")
    check(_lib.load().qsaeo_project_columns(_p(W), _p(G), D, H, ld, _stream()))


def _recipe_words(who: str, device, coef: Optional[torch.Tensor], report: Optional[torch.Tensor], T: int):
    if coef is None:
        coef = torch.empty((1,), dtype=torch.float32, device=device)
    if report is None:
        report = torch.empty((GRAD_NORM_HEAD + T,), dtype=torch.int64, device=device)
    _dev(coef, f"{who}: coef", torch.float32)
    _dev(report, f"{who}: report", torch.int64)
    if coef.numel() != 1 or coef.device != device or tuple(report.shape) != (GRAD_NORM_HEAD + T,) or report.device != device \
            or not report.is_contiguous():
        raise ValueError(f"{who}: coef must be one fp32 word and report a contiguous int64 [{GRAD_NORM_HEAD + T}] on {device}")
    return coef, report


def grad_norm(tensors, max_norm: float, coef: Optional[torch.Tensor] = None,
              report: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (coef fp32 [1], report int64 [4 + T]), both on the device: the joint L2 norm of ``tensors`` (fp32, contiguous, any
    shapes and sizes, at least one) in fp64 and the clip coefficient of ``torch.nn.utils.clip_grad_norm_(max_norm)`` as one fp32
    word.  report: the fp64 bits of the total sum of squares, the norm and the coefficient, 1 where the coefficient is not 1,
    then every tensor's sum of squares.  ``coef`` / ``report``: buffers to write into.  One call, nothing read back.  See
    qsaeo_grad_norm."""
    who = "grad_norm"
    tensors = list(tensors)
    T = len(tensors)
    if not 1 <= T <= GRAD_NORM_MAX_TENSORS:
        raise ValueError(f"{who}: takes 1 to {GRAD_NORM_MAX_TENSORS} tensors, got {T}")
    max_norm = float(max_norm)
    if not max_norm >= 0:
        raise ValueError(f"{who}: max_norm must be a number >= 0, got {max_norm}")
    for i, t in enumerate(tensors):
        _dev(t, f"{who}: tensors[{i}]")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{who}: tensors[{i}] must be a contiguous fp32 tensor, got {t.dtype} {tuple(t.shape)} with strides "
                             f"{t.stride()} (no silent copy is made)")
        if t.device != tensors[0].device:
            raise ValueError(f"{who}: tensors[{i}] is on {t.device}, tensors[0] on {tensors[0].device}")
    device = tensors[0].device
    with torch.cuda.device(device):
        coef, report = _recipe_words(who, device, coef, report, T)
        lib = _lib.load()
        counts = (C.c_int64 * T)(*[t.numel() for t in tensors])
        ptrs = (C.c_void_p * T)(*[t.data_ptr() if t.numel() else 0 for t in tensors])
        ws = _workspace(device, max(int(lib.qsaeo_grad_norm_workspace_bytes(counts, T)), 16))
        check(lib.qsaeo_grad_norm(ptrs, counts, T, max_norm, _p(coef), _p(report), _p(ws), ws.numel(), _stream()))
    return coef, report


def _recipe_streams(who: str, like: torch.Tensor, coef: Optional[torch.Tensor], emas) -> None:
    if coef is not None:
        _dev(coef, f"{who}: coef", torch.float32)
        if coef.numel() != 1 or coef.device != like.device:
            raise ValueError(f"{who}: coef must be one fp32 word on {like.device}")
    for name, e, ref in emas:
        if e is not None:
            _dev(e, f"{who}: {name}", torch.float32)
            if e.shape != ref.shape or e.device != ref.device or not e.is_contiguous():
                raise ValueError(f"{who}: {name} must be a contiguous fp32 {tuple(ref.shape)} on {ref.device} (it is updated in "
                                 "place)")


@_on_tensor_device
def adam_step_clipped(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, one_minus_b1: float, b2: float,
                      one_minus_b2: float, bc2_sqrt: float, eps: float, step_size: float,
                      coef: Optional[torch.Tensor] = None, ema: Optional[torch.Tensor] = None,
                      one_minus_decay: float = 0.0) -> None:
    """adam_step with the recipe's two optional streams: ``coef`` (one fp32 word on the device, e.g. grad_norm's) multiplies the
    gradient on its way into the step (g is not written); ``ema`` (like p, updated IN PLACE) moves towards the new p by
    ``one_minus_decay``.  With neither it is adam_step bit for bit.  See qsaeo_adam_step."""
    who = "adam_step_clipped"
    _adam_operands(who, ("p", "g", "m", "v"), (p, g, m, v))
    _recipe_streams(who, p, coef, (("ema", ema, p),))
    check(_lib.load().qsaeo_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps,
                                      step_size, _p(coef), _p(ema), one_minus_decay, _stream()))


@_on_tensor_device
def adam_step_prefilter_clipped(W: torch.Tensor, gW: torch.Tensor, mW: torch.Tensor, vW: torch.Tensor,
                                bias: Optional[torch.Tensor], gb: Optional[torch.Tensor], mb: Optional[torch.Tensor],
                                vb: Optional[torch.Tensor], one_minus_b1: float, b2: float, one_minus_b2: float,
                                bc2_sqrt: float, eps: float, step_size: float, coef: Optional[torch.Tensor] = None,
                                emaW: Optional[torch.Tensor] = None, emab: Optional[torch.Tensor] = None,
                                one_minus_decay: float = 0.0, Wq: Optional[torch.Tensor] = None,
                                meta: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """adam_step_prefilter with the recipe's two optional streams (see adam_step_clipped); ``emaW`` and ``emab`` are given
    together where there is a bias.  -> (Wq, meta), bit-identical to prefilter_pack_w of the updated W / bias.  See
    qsaeo_adam_step_prefilter."""
    who = "adam_step_prefilter_clipped"
    _adam_operands(who, ("W", "gW", "mW", "vW"), (W, gW, mW, vW))
    if W.dim() != 2 or W.numel() == 0:
        raise ValueError(f"{who}: W is {tuple(W.shape)}, expected [H >= 1, D >= 1]")
    H, D = W.shape
    quad = (bias, gb, mb, vb)
    if any(t is None for t in quad) and not all(t is None for t in quad):
        raise ValueError(f"{who}: bias, gb, mb and vb are given together or not at all")
    if bias is not None:
        _adam_operands(who, ("bias", "gb", "mb", "vb"), quad)
        if tuple(bias.shape) != (H,) or bias.device != W.device:
            raise ValueError(f"{who}: bias is {tuple(bias.shape)} on {bias.device}, W is {tuple(W.shape)} on {W.device}")
    if W.data_ptr() % 16 != 0:
        raise ValueError(f"{who}: W must be 16-byte aligned (the prefilter entry points ask for that too)")
    if (emab is not None) != (emaW is not None and bias is not None):
        raise ValueError(f"{who}: emab is given exactly where emaW and bias both are")
    _recipe_streams(who, W, coef, (("emaW", emaW, W), ("emab", emab, bias)))
    if Wq is None:
        Wq = torch.empty((H, D), dtype=torch.float16, device=W.device)
    if meta is None:
        meta = torch.empty((4,), dtype=torch.float32, device=W.device)
    _dev(Wq, f"{who}: Wq", torch.float16)
    _dev(meta, f"{who}: meta", torch.float32)
    if tuple(Wq.shape) != (H, D) or tuple(meta.shape) != (4,) or not Wq.is_contiguous() or not meta.is_contiguous() \
            or Wq.device != W.device or meta.device != W.device or Wq.data_ptr() % 16 != 0:
        raise ValueError(f"{who}: Wq must be a contiguous 16-byte aligned fp16 [{H}, {D}] and meta a contiguous fp32 [4] on "
                         f"{W.device}")
    check(_lib.load().qsaeo_adam_step_prefilter(_p(W), _p(gW), _p(mW), _p(vW), _p(bias), _p(gb), _p(mb), _p(vb), H, D,
                                                one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size, _p(coef), _p(emaW),
                                                _p(emab), one_minus_decay, _p(Wq), _p(meta), _stream()))
    return Wq, meta


# ---- trainer: batch supply and loss (csrc/trainer.hip; quantizedsae_amd.training is the user) ------------------------------------
TRAINER_LOSS_MAX_LEVELS = 8


def _chunk_rows(src: torch.Tensor, who: str):
    """src: a chunk of hidden states, [..., D] contiguous in fp32 / fp16 / bf16 -> (rows, D)."""
    _dev(src, f"{who}: src")
    if src.dtype not in MOMENTS_DTYPES:
        raise TypeError(f"{who}: src: expected fp32, fp16 or bf16, got {src.dtype}")
    if src.dim() < 2 or src.shape[-1] < 1 or not src.is_contiguous():
        raise ValueError(f"{who}: src must be contiguous [..., D >= 1], got {tuple(src.shape)} with strides {src.stride()}")
    D = src.shape[-1]
    return src.numel() // D, D


@_on_tensor_device
def rows_nan_bitmap(src: torch.Tensor) -> torch.Tensor:
    """-> int32 [ceil(rows / 32)] on the device: bit r % 32 of word r // 32 is set where row r of src [..., D] (fp32, fp16 or
    bf16; the leading dimensions are flattened) holds a NaN; inf does not count.  See qsae_rows_nan_bitmap."""
    rows, D = _chunk_rows(src, "rows_nan_bitmap")
    bits = torch.empty(((rows + 31) // 32,), dtype=torch.int32, device=src.device)
    check(_lib.load().qsae_rows_nan_bitmap(_p(src), MOMENTS_DTYPES[src.dtype], rows, D, _p(bits), _stream()))
    return bits


@_on_tensor_device
def gather_rows(src: torch.Tensor, idx: torch.Tensor, flag: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> fp32 [B, D]: out[b] = src[idx[b]].float() over the rows of src [..., D] (leading dimensions flattened), idx int64 [B]
    on the device.  An index outside the chunk gives a row of zeros and sets bit 0 of ``flag`` (int32 [1] on the device,
    zeroed by the caller); nothing is read back here.  See qsae_gather_rows."""
    rows, D = _chunk_rows(src, "gather_rows")
    _dev(idx, "gather_rows: idx", torch.int64)
    _dev(flag, "gather_rows: flag", torch.int32)
    if idx.dim() != 1 or not idx.is_contiguous() or flag.numel() != 1 or idx.device != src.device or flag.device != src.device:
        raise ValueError(f"gather_rows: idx must be a contiguous int64 [B] and flag an int32 [1] on {src.device}, got "
                         f"{tuple(idx.shape)} on {idx.device} and {tuple(flag.shape)} on {flag.device}")
    B = idx.shape[0]
    if out is None:
        out = torch.empty((B, D), dtype=torch.float32, device=src.device)
    else:
        _dev(out, "gather_rows: out", torch.float32)
        if tuple(out.shape) != (B, D) or not out.is_contiguous() or out.device != src.device:
            raise ValueError(f"gather_rows: out must be a contiguous fp32 [{B}, {D}] on {src.device}")
    check(_lib.load().qsae_gather_rows(_p(src), MOMENTS_DTYPES[src.dtype], rows, D, _p(idx), B, _p(out), _p(flag), _stream()))
    return out


@_on_tensor_device
def trainer_loss(x: torch.Tensor, recons, mode: int, coef: float, grads: Optional[torch.Tensor] = None):
    """-> (losses fp32 [n], grads fp32 [n, B, D]), both on the device: losses[i] = coef * mse(recons[i], t_i) and grads[i] its
    gradient at recons[i], t_i = x (mode 0) or the detached doubled residual chain of rq_sae (mode 1), in one pass over x and
    the n <= 8 reconstructions (fp32 [B, D], contiguous; views that start off a 16-byte boundary are fine).  ``grads``: a
    buffer to write into instead of a new one.  See qsae_trainer_loss."""
    who = "trainer_loss"
    _dev(x, f"{who}: x", torch.float32)
    if x.dim() != 2 or not x.is_contiguous() or x.shape[1] < 1:
        raise ValueError(f"{who}: x must be a contiguous fp32 [B, D >= 1], got {tuple(x.shape)} with strides {x.stride()}")
    B, D = x.shape
    recons = list(recons)
    n = len(recons)
    if not 1 <= n <= TRAINER_LOSS_MAX_LEVELS:
        raise ValueError(f"{who}: takes 1 to {TRAINER_LOSS_MAX_LEVELS} reconstructions, got {n}")
    if mode not in (0, 1):
        raise ValueError(f"{who}: mode must be 0 (every level against x) or 1 (the doubled residual chain), got {mode!r}")
    for i, r in enumerate(recons):
        _dev(r, f"{who}: recons[{i}]", torch.float32)
        if r.shape != x.shape or not r.is_contiguous() or r.device != x.device:
            raise ValueError(f"{who}: recons[{i}] is {tuple(r.shape)} on {r.device} (strides {r.stride()}), x is a contiguous "
                             f"{tuple(x.shape)} on {x.device}")
    if grads is None:
        grads = torch.empty((n, B, D), dtype=torch.float32, device=x.device)
    else:
        _dev(grads, f"{who}: grads", torch.float32)
        if tuple(grads.shape) != (n, B, D) or not grads.is_contiguous() or grads.device != x.device:
            raise ValueError(f"{who}: grads must be a contiguous fp32 [{n}, {B}, {D}] on {x.device}")
    losses = torch.empty((n,), dtype=torch.float32, device=x.device)
    if B == 0:
        return losses.fill_(float("nan")), grads             # the mean over nothing, as F.mse_loss reports it
    lib = _lib.load()
    ws = _workspace(x.device, max(int(lib.qsae_trainer_loss_workspace_bytes(n, B, D)), 16))
    rp = (C.c_void_p * n)(*[r.data_ptr() for r in recons])
    gp = (C.c_void_p * n)(*[grads.data_ptr() + i * B * D * 4 for i in range(n)])
    check(lib.qsae_trainer_loss(_p(x), rp, n, B, D, int(mode), float(coef), gp, _p(losses), _p(ws), ws.numel(), _stream()))
    return losses, grads


# ---- watch: the distributions of a list of tensors (csrc/watch.hip; quantizedsae_amd.training.watch is the user) ---------------
TENSOR_STATS_HEAD = 8
TENSOR_STATS_MAX_BINS = 256


def tensor_stats(tensors, bins: int = 64) -> torch.Tensor:
    """-> int64 [T, 8 + bins] on the device, one row per tensor of ``tensors`` (fp32, contiguous, any shapes and sizes, views
    that start off a 16-byte boundary included): words 0 .. 3 are the fp64 bits of lo, hi, mean and the sum of squared
    deviations over the finite elements, words 4 .. 6 n_finite, n_nonfinite and n_zero, words 8 .. the counts of
    ``torch.histc(finite elements, bins, lo, hi)`` as the CPU computes them.  One call for the whole list, nothing read back.
    See qsae_tensor_stats; ``quantizedsae_amd.training.tensor_stats`` gives the parsed form."""
    who = "tensor_stats"
    tensors = list(tensors)
    bins = int(bins)
    if not 1 <= bins <= TENSOR_STATS_MAX_BINS:
        raise ValueError(f"{who}: bins must be in 1 .. {TENSOR_STATS_MAX_BINS}, got {bins}")
    for i, t in enumerate(tensors):
        _dev(t, f"{who}: tensors[{i}]")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{who}: tensors[{i}] must be a contiguous fp32 tensor, got {t.dtype} {tuple(t.shape)} with strides "
                             f"{t.stride()} (no silent copy is made)")
        if t.device != tensors[0].device:
            raise ValueError(f"{who}: tensors[{i}] is on {t.device}, tensors[0] on {tensors[0].device}")
    T = len(tensors)
    device = tensors[0].device if T else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(device):
        result = torch.zeros((T, TENSOR_STATS_HEAD + bins), dtype=torch.int64, device=device)
        if sum(t.numel() for t in tensors) == 0:
            return result
        lib = _lib.load()
        counts = (C.c_int64 * T)(*[t.numel() for t in tensors])
        ptrs = (C.c_void_p * T)(*[t.data_ptr() if t.numel() else 0 for t in tensors])
        ws = _workspace(device, max(int(lib.qsae_tensor_stats_workspace_bytes(counts, T)), 16))
        check(lib.qsae_tensor_stats(ptrs, counts, T, 0, bins, _p(result), _p(ws), ws.numel(), _stream()))
    return result


# ---- activity: per-unit firing counts of a model in training (csrc/activity.hip; quantizedsae_amd.training.activity is the user) ----
ACTIVITY_HEAD = 8
ACTIVITY_BINS = 34
ACTIVITY_MAX_SEGMENTS = 16


def _activity_state(who: str, **state) -> int:
    """fired / last / base: contiguous int64 [H] on one device -> H"""
    H = dev = None
    for name, t in state.items():
        if t is None:
            continue
        _dev(t, f"{who}: {name}", torch.int64)
        if t.dim() != 1 or not t.is_contiguous() or t.numel() < 1:
            raise ValueError(f"{who}: {name} must be a contiguous int64 [H >= 1], got {tuple(t.shape)} with strides {t.stride()}")
        if H is None:
            H, dev = t.numel(), t.device
        elif t.numel() != H or t.device != dev:
            raise ValueError(f"{who}: {name} is [{t.numel()}] on {t.device}, expected [{H}] on {dev}")
    return H


def _activity_stamp(who: str, stamp) -> int:
    stamp = int(stamp)
    if stamp < 1:
        raise ValueError(f"{who}: stamp must be >= 1, got {stamp}")
    return stamp


@_on_tensor_device
def activity_add_compact(idx: torch.Tensor, val: Optional[torch.Tensor], stamp: int, fired: torch.Tensor,
                         last: torch.Tensor) -> None:
    """fired[h] += the rows whose entry h is active (val > 0; every listed entry when val is None) and
    last[h] = max(last[h], stamp) for those units, in one pass over idx int32 [B, k].  fired / last int64 [H].  See
    qsae_activity_add_compact."""
    who = "activity_add_compact"
    _dev(idx, f"{who}: idx", torch.int32)
    if idx.dim() != 2:
        raise ValueError(f"{who}: idx must be [B, k], got {tuple(idx.shape)}")
    B, k = idx.shape
    if val is not None:
        _dev(val, f"{who}: val", torch.float32)
        if val.shape != idx.shape:
            raise ValueError(f"{who}: val is {tuple(val.shape)}, idx {tuple(idx.shape)}")
        val = val.contiguous()
    H = _activity_state(who, fired=fired, last=last)
    check(_lib.load().qsae_activity_add_compact(_p(idx.contiguous()), _p(val), B, k, H, _activity_stamp(who, stamp), _p(fired),
                                                _p(last), _stream()))


@_on_tensor_device
def activity_add_bits(zbits: torch.Tensor, index: Optional[torch.Tensor], stamp: int, fired: torch.Tensor,
                      last: torch.Tensor) -> None:
    """The same from packed bits: zbits int32 [B, words] (a column slice of a wider tensor is fine), ``index`` (int32 / int64
    [32 * words]) maps a packed position to its unit, -1 = pad slot; None = identity (32 * words <= H).  An int32 contiguous
    ``index`` is passed through as it is.  See qsae_activity_add_bits."""
    who = "activity_add_bits"
    _dev(zbits, f"{who}: zbits", torch.int32)
    if zbits.dim() != 2:
        raise ValueError(f"{who}: zbits must be [B, words], got {tuple(zbits.shape)}")
    B, words = zbits.shape
    if zbits.stride(1) != 1:
        zbits = zbits.contiguous()
    index = _packed_index_arg(index, 32 * words)
    H = _activity_state(who, fired=fired, last=last)
    check(_lib.load().qsae_activity_add_bits(_p(zbits), zbits.stride(0) if B else words, B, 32 * words, _p(index), H,
                                             _activity_stamp(who, stamp), _p(fired), _p(last), _stream()))


@_on_tensor_device
def activity_add_dense(latent: torch.Tensor, stamp: int, fired: torch.Tensor, last: torch.Tensor) -> None:
    """The same from a dense latent fp32 [B, H] with unit column stride (a row stride above H is fine): active = latent > 0.
    See qsae_activity_add_dense."""
    who = "activity_add_dense"
    _dev(latent, f"{who}: latent", torch.float32)
    H = _activity_state(who, fired=fired, last=last)
    if latent.dim() != 2 or latent.shape[1] != H:
        raise ValueError(f"{who}: latent must be [B, {H}], got {tuple(latent.shape)}")
    if latent.stride(1) != 1:
        latent = latent.contiguous()
    B = latent.shape[0]
    check(_lib.load().qsae_activity_add_dense(_p(latent), latent.stride(0) if B else H, B, H, _activity_stamp(who, stamp),
                                              _p(fired), _p(last), _stream()))


@_on_tensor_device
def activity_summary(fired: torch.Tensor, base: Optional[torch.Tensor], last: torch.Tensor, clock: int, window: int,
                     seg_sizes=(), advance: bool = True, dead_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> int64 [1 + n_seg, 8 + 34] on the device: per block (all units, then the consecutive segments of ``seg_sizes``) the
    words units, never, dead, silent, sum of interval counts, sum of fired, largest interval count, 0, and the 34 octave bins
    of the interval counts fired - base.  ``advance`` writes base = fired; ``dead_out`` (int32 [H]) receives the dead units
    in ascending order in its first ``result[0, 2]`` entries.  Nothing is read back.  See qsae_activity_summary."""
    who = "activity_summary"
    H = _activity_state(who, fired=fired, last=last, base=base)
    seg_sizes = [int(s) for s in seg_sizes]
    if len(seg_sizes) > ACTIVITY_MAX_SEGMENTS:
        raise ValueError(f"{who}: at most {ACTIVITY_MAX_SEGMENTS} segments, got {len(seg_sizes)}")
    if seg_sizes and (min(seg_sizes) < 0 or sum(seg_sizes) != H):
        raise ValueError(f"{who}: the segment sizes {seg_sizes} must be >= 0 and add up to H = {H}")
    clock, window = int(clock), int(window)
    if clock < 0 or window < 1:
        raise ValueError(f"{who}: clock must be >= 0 and window >= 1, got clock = {clock}, window = {window}")
    if dead_out is not None:
        _dev(dead_out, f"{who}: dead_out", torch.int32)
        if dead_out.dim() != 1 or dead_out.numel() != H or not dead_out.is_contiguous() or dead_out.device != fired.device:
            raise ValueError(f"{who}: dead_out must be a contiguous int32 [{H}] on {fired.device}")
    lib = _lib.load()
    result = torch.empty((1 + len(seg_sizes), ACTIVITY_HEAD + ACTIVITY_BINS), dtype=torch.int64, device=fired.device)
    ws = _workspace(fired.device, max(int(lib.qsae_activity_summary_workspace_bytes(H)), 16))
    sizes = (C.c_int32 * len(seg_sizes))(*seg_sizes) if seg_sizes else None
    check(lib.qsae_activity_summary(_p(fired), _p(base), _p(last), H, clock, window, sizes, len(seg_sizes), int(bool(advance)),
                                    _p(result), _p(dead_out), _p(ws), ws.numel(), _stream()))
    return result


# ---- resampling: revive dead units from high-loss rows (csrc/resample.hip; quantizedsae_amd.training.resample is the user) ----
RESAMPLE_MAX_D = 4096
RESAMPLE_REPORT_WORDS = 8


def resample_supported(D: int) -> bool:
    """The resampling kernels take input_dim a multiple of 4 up to 4096"""
    return 4 <= D <= RESAMPLE_MAX_D and D % 4 == 0


def _resample_rows(who: str, name: str, t: torch.Tensor, D: Optional[int] = None) -> torch.Tensor:
    """fp32 [N, D] with unit column stride (a row stride above D is read in place)"""
    _dev(t, f"{who}: {name}", torch.float32)
    if t.dim() != 2 or (D is not None and t.shape[1] != D):
        raise ValueError(f"{who}: {name} must be fp32 [N, {D if D is not None else 'D'}], got {tuple(t.shape)}")
    if not resample_supported(t.shape[1]):
        raise ValueError(f"{who}: the kernels take D a multiple of 4 up to {RESAMPLE_MAX_D}, got {t.shape[1]}")
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def _resample_vec(who: str, name: str, t: torch.Tensor, dtype, n: Optional[int] = None) -> int:
    _dev(t, f"{who}: {name}", dtype)
    if t.dim() != 1 or not t.is_contiguous() or (n is not None and t.numel() != n):
        raise ValueError(f"{who}: {name} must be a contiguous {dtype} [{n if n is not None else 'n'}], got {tuple(t.shape)} "
                         f"with strides {t.stride()}")
    return t.numel()


@_on_tensor_device
def resample_row_weights(x: torch.Tensor, recon: torch.Tensor) -> torch.Tensor:
    """-> w fp64 [N]: the squared loss of every row, w_r = (sum_d (x[r,d] - recon[r,d])^2)^2 in a fixed order, 0 where the sum
    is not finite.  See qsae_resample_row_weights."""
    who = "resample_row_weights"
    x = _resample_rows(who, "x", x)
    N, D = x.shape
    recon = _resample_rows(who, "recon", recon, D)
    if recon.shape[0] != N or recon.device != x.device:
        raise ValueError(f"{who}: recon is {tuple(recon.shape)} on {recon.device}, x {tuple(x.shape)} on {x.device}")
    w = torch.empty((N,), dtype=torch.float64, device=x.device)
    check(_lib.load().qsae_resample_row_weights(_p(x), x.stride(0) if N else D, _p(recon), recon.stride(0) if N else D, N, D,
                                                _p(w), _stream()))
    return w


@_on_tensor_device
def resample_draw(w: torch.Tensor, u: torch.Tensor):
    """-> (rows int32 [n], report int64 [8]): one row per dead unit with probability proportional to w (fp64 [N]) from the
    uniforms u (fp64 [n] in [0, 1)); rows[j] = -1 when the total weight is 0 or not finite, -2 when an earlier unit drew the
    same row.  See qsae_resample_draw."""
    who = "resample_draw"
    N = _resample_vec(who, "w", w, torch.float64)
    n = _resample_vec(who, "u", u, torch.float64)
    if N < 1:
        raise ValueError(f"{who}: w must hold at least one row")
    if u.device != w.device:
        raise ValueError(f"{who}: u is on {u.device}, w on {w.device}")
    rows = torch.empty((n,), dtype=torch.int32, device=w.device)
    report = torch.zeros((RESAMPLE_REPORT_WORDS,), dtype=torch.int64, device=w.device)
    if n == 0:
        return rows, report
    lib = _lib.load()
    ws = _workspace(w.device, max(int(lib.qsae_resample_draw_workspace_bytes(N)), 16))
    check(lib.qsae_resample_draw(_p(w), N, _p(u), n, _p(rows), _p(report), _p(ws), ws.numel(), _stream()))
    return rows, report


def _resample_weights(who: str, W_enc: torch.Tensor):
    _dev(W_enc, f"{who}: W_enc", torch.float32)
    if W_enc.dim() != 2 or not W_enc.is_contiguous():
        raise ValueError(f"{who}: W_enc must be a contiguous fp32 [H, D], got {tuple(W_enc.shape)} with strides {W_enc.stride()} "
                         "(it is written in place: no copy is made)")
    H, D = W_enc.shape
    if not resample_supported(D):
        raise ValueError(f"{who}: the kernels take D a multiple of 4 up to {RESAMPLE_MAX_D}, got {D}")
    return H, D


def _resample_bits(who: str, n_bits) -> int:
    n_bits = int(n_bits)
    if not 1 <= n_bits <= 8:
        raise ValueError(f"{who}: n_bits must be 1 .. 8, got {n_bits}")
    return n_bits


def _resample_same(who: str, name: str, t: Optional[torch.Tensor], like: torch.Tensor, dtype=torch.float32) -> None:
    """an operand written in place (or a moment of one): the dtype, shape and device of ``like``, contiguous; None passes"""
    if t is None:
        return
    _dev(t, f"{who}: {name}", dtype)
    if tuple(t.shape) != tuple(like.shape) or not t.is_contiguous() or t.device != like.device:
        raise ValueError(f"{who}: {name} must be a contiguous {dtype} {tuple(like.shape)} on {like.device}, got {tuple(t.shape)} "
                         f"with strides {t.stride()} on {t.device}")


@_on_tensor_device
def resample_alive_stats(W_enc: torch.Tensor, logits: Optional[torch.Tensor], dead: torch.Tensor, n_bits: int = 8) -> torch.Tensor:
    """-> stats fp64 [2]: the mean encoder-row norm of the units not in ``dead`` (int32 [n], ascending) and, with ``logits``
    (fp32 [H, D n_bits]), the mean |logit| of the same rows (0.0 without); over every unit when none is alive.  See
    qsae_resample_alive_stats."""
    who = "resample_alive_stats"
    H, D = _resample_weights(who, W_enc)
    n = _resample_vec(who, "dead", dead, torch.int32)
    if n > H:
        raise ValueError(f"{who}: {n} dead units of {H}")
    unit_abs = None
    if logits is not None:
        n_bits = _resample_bits(who, n_bits)
        _dev(logits, f"{who}: logits", torch.float32)
        if tuple(logits.shape) != (H, D * n_bits) or not logits.is_contiguous():
            raise ValueError(f"{who}: logits must be a contiguous fp32 [{H}, {D * n_bits}], got {tuple(logits.shape)}")
        unit_abs = torch.empty((H,), dtype=torch.float64, device=W_enc.device)
    unit_norm = torch.empty((H,), dtype=torch.float64, device=W_enc.device)
    stats = torch.empty((2,), dtype=torch.float64, device=W_enc.device)
    check(_lib.load().qsae_resample_alive_stats(_p(W_enc), H, D, _p(logits), int(n_bits) if logits is not None else 0,
                                                _p(dead) if n else C.c_void_p(0), n, _p(unit_norm), _p(unit_abs), _p(stats),
                                                _stream()))
    return stats


def _resample_write_args(who, dead, rows, x, dec_bias, stats, W_enc, b_enc, dec, dec_shape, moments, last, rows_seen, report):
    H, D = _resample_weights(who, W_enc)
    n = _resample_vec(who, "dead", dead, torch.int32)
    _resample_vec(who, "rows", rows, torch.int32, n)
    if n > H:
        raise ValueError(f"{who}: {n} dead units of {H}")
    x = _resample_rows(who, "x", x, D)
    if x.shape[0] < 1:
        raise ValueError(f"{who}: x holds no row")
    _resample_vec(who, "dec_bias", dec_bias, torch.float32, D)
    _resample_vec(who, "stats", stats, torch.float64, 2)
    _resample_vec(who, "b_enc", b_enc, torch.float32, H)
    _resample_vec(who, "report", report, torch.int64, RESAMPLE_REPORT_WORDS)
    _dev(dec, f"{who}: dec", torch.float32)
    if tuple(dec.shape) != dec_shape(H, D) or not dec.is_contiguous():
        raise ValueError(f"{who}: dec must be a contiguous fp32 {dec_shape(H, D)}, got {tuple(dec.shape)}")
    moments = list(moments) if moments is not None else [None] * 6
    if len(moments) != 6:
        raise ValueError(f"{who}: moments must be (m_We, v_We, m_be, v_be, m_dec, v_dec), each a tensor or None")
    for name, t, like in zip(("m_We", "v_We", "m_be", "v_be", "m_dec", "v_dec"), moments, (W_enc, W_enc, b_enc, b_enc, dec, dec)):
        _resample_same(who, name, t, like)
    if last is not None:
        _resample_vec(who, "last", last, torch.int64, H)
    rows_seen = int(rows_seen)
    if rows_seen < 0:
        raise ValueError(f"{who}: rows_seen = {rows_seen}")
    for name, t in (("dead", dead), ("rows", rows), ("x", x), ("dec_bias", dec_bias), ("stats", stats), ("b_enc", b_enc),
                    ("dec", dec), ("report", report), ("last", last)):
        if t is not None and t.device != W_enc.device:
            raise ValueError(f"{who}: {name} is on {t.device}, W_enc on {W_enc.device}")
    return n, x, H, D, moments, rows_seen


@_on_tensor_device
def resample_write_table(W_enc: torch.Tensor, b_enc: torch.Tensor, dec: torch.Tensor, dead: torch.Tensor, rows: torch.Tensor,
                         x: torch.Tensor, dec_bias: torch.Tensor, stats: torch.Tensor, report: torch.Tensor, moments=None,
                         last: Optional[torch.Tensor] = None, rows_seen: int = 0, encoder_scale: float = 0.2) -> None:
    """Point every dead unit that owns a row at it, in place: W_enc [H, D] row, b_enc [H] entry and column h of ``dec``
    [D, H] (the nn.Linear layout of BaselineSparseAutoencoder.decoder.weight); ``moments`` = (m_We, v_We, m_be, v_be, m_dec,
    v_dec), each a tensor or None, are zeroed at the written positions; ``last`` [H] receives rows_seen.  ``report`` (from
    resample_draw) gains the revived and degenerate counts.  See qsae_resample_write_table."""
    who = "resample_write_table"
    n, x, H, D, moments, rows_seen = _resample_write_args(who, dead, rows, x, dec_bias, stats, W_enc, b_enc, dec,
                                                           lambda H, D: (D, H), moments, last, rows_seen, report)
    if n == 0:
        return
    check(_lib.load().qsae_resample_write_table(_p(dead), _p(rows), n, _p(x), x.stride(0), x.shape[0], D, H, _p(dec_bias),
                                                _p(stats), float(encoder_scale), _p(W_enc), _p(b_enc), _p(dec),
                                                *[_p(m) for m in moments], _p(last), rows_seen, _p(report), _stream()))


@_on_tensor_device
def resample_write_binary(W_enc: torch.Tensor, b_enc: torch.Tensor, dec: torch.Tensor, dead: torch.Tensor, rows: torch.Tensor,
                          x: torch.Tensor, dec_bias: torch.Tensor, stats: torch.Tensor, report: torch.Tensor, n_bits: int,
                          moments=None, last: Optional[torch.Tensor] = None, rows_seen: int = 0, encoder_scale: float = 0.2,
                          logit_scale: Optional[float] = None) -> None:
    """The same for BinarySAE: ``dec`` is the logit matrix [H, D n_bits]; row h receives +-L per bit of the row's direction
    quantized to n_bits two's-complement integers, L = logit_scale or, when None, stats[1] (the alive rows' mean |logit|).
    See qsae_resample_write_binary."""
    who = "resample_write_binary"
    n_bits = _resample_bits(who, n_bits)
    n, x, H, D, moments, rows_seen = _resample_write_args(who, dead, rows, x, dec_bias, stats, W_enc, b_enc, dec,
                                                           lambda H, D: (H, D * n_bits), moments, last, rows_seen, report)
    if n == 0:
        return
    check(_lib.load().qsae_resample_write_binary(_p(dead), _p(rows), n, _p(x), x.stride(0), x.shape[0], D, H, n_bits,
                                                 _p(dec_bias), _p(stats), float(encoder_scale), int(logit_scale is not None),
                                                 float(logit_scale) if logit_scale is not None else 0.0, _p(W_enc), _p(b_enc),
                                                 _p(dec), *[_p(m) for m in moments], _p(last), rows_seen, _p(report), _stream()))


# ---- AuxK: the dead units' own top-k and the normalised auxiliary loss (csrc/auxk.hip, include/qsae_ext.h) -----------------
ENCODE_TOPK_UNITS_MAX_K = 64


@_on_tensor_device
def encode_topk_units(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], units: torch.Tensor, k: int):
    """-> (idx int32 [B, k] of unit ids, val fp32 [B, k]): the k largest encoder pre-activations of every row among the units
    listed in ``units`` (int32 [n], ascending, distinct, on the device), ordered by value descending, then unit ascending.  W's
    rows are read in place: no gathered copy, no [B, n] tensor.  See qsaex_encode_topk_units."""
    who = "encode_topk_units"
    x, W = _f32c(x, "x"), _f32c(W, "W")
    _dev(units, f"{who}: units", torch.int32)
    if x.dim() != 2 or W.dim() != 2 or units.dim() != 1 or x.shape[1] != W.shape[1]:
        raise ValueError(f"{who}: x is {tuple(x.shape)}, W {tuple(W.shape)}, units {tuple(units.shape)}; expected [B, D], [H, D], [n]")
    units = units.contiguous()
    B, D = x.shape
    H, n = W.shape[0], units.shape[0]
    k = int(k)
    if not 1 <= k <= ENCODE_TOPK_UNITS_MAX_K:
        raise ValueError(f"{who}: k = {k} is outside 1 .. {ENCODE_TOPK_UNITS_MAX_K}, the width of the kernel's lists")
    if k > n:
        raise ValueError(f"{who}: k = {k} exceeds the {n} listed units")
    if D % 4 != 0:
        raise ValueError(f"{who}: D = {D} must be a multiple of 4")
    b = _f32c(bias, "bias") if bias is not None else None
    if b is not None and tuple(b.shape) != (H,):
        raise ValueError(f"{who}: bias is {tuple(b.shape)}, expected [{H}]")
    idx = torch.empty((B, k), dtype=torch.int32, device=x.device)
    val = torch.empty((B, k), dtype=torch.float32, device=x.device)
    if B == 0:
        return idx, val
    lib = _lib.load()
    ws = _workspace(x.device, int(lib.qsaex_encode_topk_units_workspace_bytes(B, D, n, k)))
    check(lib.qsaex_encode_topk_units(_p(x), D, _p(W), D, _p(b), B, D, H, _p(units), n, k, _p(idx), _p(val), _p(ws), ws.numel(),
                                      _stream()))
    return idx, val


@_on_tensor_device
def auxk_loss(x: torch.Tensor, recon: torch.Tensor, aux: torch.Tensor, coef: float, sums: Optional[torch.Tensor] = None):
    """-> (loss fp32 0-d, grad fp32 [B, D]), both on the device: loss = coef * |aux - e|^2 / |e - mean_rows(e)|^2 with
    e = x - recon, and its gradient at ``aux`` (the only operand that has one); 0 and zeros when the denominator is 0.
    x, recon, aux: fp32 [B, D], contiguous (views that start off a 16-byte boundary are fine).  ``sums``: an fp64 [2] device
    tensor that receives (numerator, denominator).  Fixed summation order, nothing read back.  See qsaex_auxk_loss."""
    who = "auxk_loss"
    for name, t in (("x", x), ("recon", recon), ("aux", aux)):
        _dev(t, f"{who}: {name}", torch.float32)
        if t.dim() != 2 or t.shape != x.shape or not t.is_contiguous() or t.device != x.device or t.shape[1] < 1:
            raise ValueError(f"{who}: {name} is {tuple(t.shape)} on {t.device} (strides {t.stride()}); expected contiguous fp32 "
                             f"[B, D >= 1] tensors of one shape on one device")
    if sums is not None:
        _dev(sums, f"{who}: sums", torch.float64)
        if tuple(sums.shape) != (2,) or not sums.is_contiguous() or sums.device != x.device:
            raise ValueError(f"{who}: sums must be a contiguous fp64 [2] on {x.device}")
    B, D = x.shape
    loss = torch.zeros((), dtype=torch.float32, device=x.device)
    grad = torch.empty((B, D), dtype=torch.float32, device=x.device)
    if B == 0:
        return loss, grad
    lib = _lib.load()
    ws = _workspace(x.device, int(lib.qsaex_auxk_loss_workspace_bytes(B, D)))
    check(lib.qsaex_auxk_loss(_p(x), _p(recon), _p(aux), B, D, float(coef), _p(loss), _p(grad), _p(sums), _p(ws), ws.numel(),
                              _stream()))
    return loss, grad


# ---- sparsity-fidelity curve (include/qsae_curve.h) ---------------------------------------------------------------------
PREFIX_ERRORS_MAX_K = 256
PREFIX_ERRORS_MAX_POINTS = 16
PREFIX_ERRORS_MAX_D = 4096


@_on_tensor_device
def prefix_errors(x: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, ks, decoder, dec_bias: Optional[torch.Tensor],
                  group_rows: int, sums: torch.Tensor, counts: torch.Tensor, recon_out: Optional[torch.Tensor] = None) -> None:
    """sums fp64 [len(ks)] += the squared reconstruction error of the rows of x [B, D] at every k' of ``ks`` (ascending,
    distinct, 0 <= k' <= K), each decoded from the first k' entries of the rank-ordered lists idx int32 / val fp32 [B, K];
    counts int64 [2] += (rows kept, rows skipped), groups of ``group_rows`` rows holding a NaN being skipped as in
    dataset_moments_add.  ``decoder`` = ("packed", packed uint8 [H, row_bytes], n_bits, step) or ("table", fp32 [H, D],
    scale).  recon_out: fp32 [len(ks), B, D] that receives every point's reconstruction, or None.  Each point is bit for bit
    the sparse decoder's result on the truncated lists.  See qsaec_prefix_errors_binary / _table."""
    who = "prefix_errors"
    _dev(x, f"{who}: x", torch.float32)
    _dev(idx, f"{who}: idx", torch.int32)
    _dev(val, f"{who}: val", torch.float32)
    if x.dim() != 2 or idx.dim() != 2 or idx.shape != val.shape or idx.shape[0] != x.shape[0]:
        raise ValueError(f"{who}: x is {tuple(x.shape)}, idx {tuple(idx.shape)}, val {tuple(val.shape)}; expected [B, D], [B, K], [B, K]")
    for name, t in (("x", x), ("idx", idx), ("val", val)):
        if not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"{who}: {name} must be contiguous and on {x.device}")
    B, D = x.shape
    K = idx.shape[1]
    ks = [int(k) for k in ks]
    n_ks = len(ks)
    if not 1 <= n_ks <= PREFIX_ERRORS_MAX_POINTS:
        raise ValueError(f"{who}: {n_ks} points; 1 .. {PREFIX_ERRORS_MAX_POINTS} are supported")
    if K > PREFIX_ERRORS_MAX_K:
        raise ValueError(f"{who}: K = {K} exceeds {PREFIX_ERRORS_MAX_K}")
    if ks[0] < 0 or ks[-1] > K or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"{who}: ks = {ks} must be ascending and distinct within 0 .. K = {K}")
    if D < 4 or D % 4 != 0 or D > PREFIX_ERRORS_MAX_D:
        raise ValueError(f"{who}: D = {D} must be a positive multiple of 4 up to {PREFIX_ERRORS_MAX_D}")
    group_rows = int(group_rows)
    if group_rows < 1:
        raise ValueError(f"{who}: group_rows must be >= 1, got {group_rows}")
    _dev(sums, f"{who}: sums", torch.float64)
    _dev(counts, f"{who}: counts", torch.int64)
    if tuple(sums.shape) != (n_ks,) or tuple(counts.shape) != (2,) or not sums.is_contiguous() or not counts.is_contiguous() \
            or sums.device != x.device or counts.device != x.device:
        raise ValueError(f"{who}: state: expected contiguous sums fp64 [{n_ks}] and counts int64 [2] on {x.device}")
    if recon_out is not None:
        _dev(recon_out, f"{who}: recon_out", torch.float32)
        if tuple(recon_out.shape) != (n_ks, B, D) or not recon_out.is_contiguous() or recon_out.device != x.device:
            raise ValueError(f"{who}: recon_out must be a contiguous fp32 [{n_ks}, {B}, {D}] on {x.device}")
    db = _f32c(dec_bias, "dec_bias") if dec_bias is not None else None
    if db is not None and tuple(db.shape) != (D,):
        raise ValueError(f"{who}: dec_bias is {tuple(db.shape)}, expected [{D}]")
    lib = _lib.load()
    if decoder[0] == "packed":
        dict_t = _dev(decoder[1], f"{who}: packed", torch.uint8)
        n_bits = int(decoder[2])
        if not 1 <= n_bits <= 8:
            raise ValueError(f"{who}: n_bits = {n_bits} is outside 1 .. 8")
        if dict_t.dim() != 2 or dict_t.shape[1] != binary_row_bytes(D, n_bits) or not dict_t.is_contiguous():
            raise ValueError(f"{who}: packed is {tuple(dict_t.shape)}, expected contiguous [H, {binary_row_bytes(D, n_bits)}]")
        fn, size = lib.qsaec_prefix_errors_binary, lib.qsaec_prefix_errors_binary_workspace_bytes
        dargs = (_p(dict_t), dict_t.shape[0], D, n_bits, float(decoder[3]))
    elif decoder[0] == "table":
        dict_t = _f32c(decoder[1], "table")
        if dict_t.dim() != 2 or dict_t.shape[1] != D:
            raise ValueError(f"{who}: table is {tuple(dict_t.shape)}, expected [H, {D}]")
        fn, size = lib.qsaec_prefix_errors_table, lib.qsaec_prefix_errors_table_workspace_bytes
        dargs = (_p(dict_t), dict_t.shape[0], D, float(decoder[2]))
    else:
        raise ValueError(f"{who}: decoder must be ('packed', packed, n_bits, step) or ('table', table, scale)")
    if dict_t.device != x.device:
        raise ValueError(f"{who}: the dictionary must be on {x.device}")
    if B == 0:
        return
    ws = _workspace(x.device, max(int(size(B, n_ks, group_rows)), 16))
    karr = (C.c_int * n_ks)(*ks)                              # the one host array: read before the call returns
    check(fn(_p(x), _p(idx), _p(val), B, K, *dargs, _p(db), C.cast(karr, C.c_void_p), n_ks, group_rows, _p(sums), _p(counts), _p(recon_out), _p(ws),
             ws.numel(), _stream()))


# ---- the multi-level objectives of the top-k SAEs: what their wrappers share ------------------------------------------------
# Four families (nested levels, Multi-TopK points, ragged BatchTopK rows, nested levels over ragged rows) with one decoder, one
# row gradient and one pair of unit gradients between them.  The public names below say which family; the checks, their
# order, their texts and every allocation live here once.
NESTED_MAX_LEVELS = 8
MULTIK_MAX_POINTS = 8


def _ascending_ints(seq, end: int, who: str, name: str, noun: str, limit: int, end_name: str, end_max: Optional[int] = None):
    """``seq`` as a list of ints: 1 .. ``limit`` whole numbers, 0 < seq[0] < ... < seq[-1] == end; ``end`` itself within
    1 .. end_max where that is given."""
    try:
        out = [int(b) for b in seq]
    except TypeError:
        raise ValueError(f"{who}: {name} must be a sequence of ints, got {seq!r}") from None
    if any(isinstance(b, bool) or int(b) != b for b in seq):
        raise ValueError(f"{who}: {name} must be whole numbers, got {list(seq)!r}")
    if not 1 <= len(out) <= limit:
        raise ValueError(f"{who}: {len(out)} {noun}; 1 .. {limit} are supported")
    if end_max is not None and not 1 <= int(end) <= end_max:
        raise ValueError(f"{who}: {end_name} = {int(end)} is outside 1 .. {end_max}")
    if out[0] < 1 or any(b <= a for a, b in zip(out, out[1:])) or out[-1] != int(end):
        raise ValueError(f"{who}: {name} = {out} must be ascending and distinct, start above 0 and end at {end_name} = {int(end)}")
    return out


def nested_bounds(bounds, H: int, who: str = "nested_bounds"):
    """``bounds`` as a list of ints after the checks of qsae_nested.h: 1 .. 8 levels, 0 < bounds[0] < ... < bounds[-1] == H."""
    return _ascending_ints(bounds, H, who, "bounds", "levels", NESTED_MAX_LEVELS, "hidden_dim")


def multik_points(ks, K: int, who: str = "multik_points"):
    """``ks`` as a list of ints after the checks of qsae_multik.h: 1 .. 8 points, 0 < ks[0] < ... < ks[-1] == K <= 256."""
    return _ascending_ints(ks, K, who, "ks", "points", MULTIK_MAX_POINTS, "the list width K", TRAIN_MAX_K)


class _Levels(NamedTuple):
    """How a family names and validates its host array of levels (unit bounds, ending at H) or points (rank prefixes,
    ending at K)."""
    validate: Callable
    by_rank: bool
    noun: str                    # "level" / "point"
    grads: str                   # "g_levels" / "g_points"
    k: str                       # what the messages call the list length
    unit_prechecks: bool         # the packed unit gradient tests ranks, H >= 1 and B * k before the array
    unit_symbol: str             # of the unit gradients, {} = "" (packed) or "_table"


class _Decoder(NamedTuple):
    symbol: str                  # of the C ABI, without _binary / _table
    ragged: bool                 # takes counts: row r stops after counts[r] entries
    levels: Optional[_Levels]    # None: one reconstruction [B, D]
    below: bool                  # also returns counts_below [L, B]


class _RowGrad(NamedTuple):
    symbol: str
    ragged: bool
    need_2d: bool                # refuses an idx that is not 2-D in words of its own
    levels: _Levels


_NESTED = _Levels(nested_bounds, False, "level", "g_levels", "k", False, "qsaen_train{}_unit_grad_nested")
_MULTIK = _Levels(multik_points, True, "point", "g_points", "K", True, "qsaek_train{}_unit_grad_multik")
_DECODE_NESTED = _Decoder("qsaen_decode_nested", False, _NESTED, False)
_DECODE_MULTIK = _Decoder("qsaek_decode_multik", False, _MULTIK, False)
_DECODE_RAGGED = _Decoder("qsaeb_decode_ragged", True, None, False)
_DECODE_NESTED_RAGGED = _Decoder("qsaem_decode_nested_ragged", True, _NESTED, True)
_ROW_NESTED = _RowGrad("qsaen_row_grad_nested", False, False, _NESTED)
_ROW_MULTIK = _RowGrad("qsaek_row_grad_multik", False, True, _MULTIK)
_ROW_NESTED_RAGGED = _RowGrad("qsaem_row_grad_nested_ragged", True, False, _NESTED)

def _bounds_arg(bounds):
    return C.cast((C.c_int * len(bounds))(*bounds), C.c_void_p)      # a host array: read before the call returns


def _nested_lists(who: str, idx, val):
    _dev(idx, f"{who}: idx", torch.int32)
    _dev(val, f"{who}: val", torch.float32)
    if idx.dim() != 2 or idx.shape != val.shape or val.device != idx.device:
        raise ValueError(f"{who}: idx is {tuple(idx.shape)}, val {tuple(val.shape)}; expected two [B, k] tensors on one device")
    if idx.shape[1] > TRAIN_MAX_K:
        raise ValueError(f"{who}: k = {idx.shape[1]} exceeds {TRAIN_MAX_K}")
    return idx.contiguous(), val.contiguous()


def _nested_D(who: str, D: int) -> None:
    if D < 4 or D % 4 != 0 or D > TRAIN_MAX_D:
        raise ValueError(f"{who}: D = {D} must be a positive multiple of 4 up to {TRAIN_MAX_D}")


def _sparse_dictionary(who: str, dictionary, D, n_bits, device):
    """The dictionary operand of a sparse decoder -> (kind, dictionary, H, D, n_bits): "binary" for packed uint8
    [H, row_bytes] with D and n_bits given, "table" (n_bits None) for fp32 [H, D]."""
    if n_bits is None:
        table = _f32c(dictionary, "table")
        if table.dim() != 2 or table.device != device:
            raise ValueError(f"{who}: table is {tuple(table.shape)} on {table.device}, expected [H, D] on {device}")
        H, D = table.shape
        _nested_D(who, D)
        return "table", table, H, D, None
    packed = _dev(dictionary, f"{who}: packed", torch.uint8)
    D, n_bits = int(D), int(n_bits)
    _nested_D(who, D)
    if not 1 <= n_bits <= 8:
        raise ValueError(f"{who}: n_bits = {n_bits} is outside 1 .. 8")
    if packed.dim() != 2 or packed.shape[1] != binary_row_bytes(D, n_bits) or not packed.is_contiguous() or packed.device != device:
        raise ValueError(f"{who}: packed is {tuple(packed.shape)}, expected contiguous [H, {binary_row_bytes(D, n_bits)}] on {device}")
    return "binary", packed, packed.shape[0], D, n_bits


def _decode_sparse(fam: _Decoder, who: str, idx, val, counts, dictionary, D, n_bits, mult: float, bias, levels):
    """Every sparse decoder of the four families: the lists, the dictionary, the levels or points, the bias -- in this order,
    the bias after the levels -- and one call."""
    if fam.ragged:
        idx, val, counts = _batch_lists(who, idx, val, counts)
    else:
        idx, val = _nested_lists(who, idx, val)
    kind, dictionary, H, D, n_bits = _sparse_dictionary(who, dictionary, D, n_bits, idx.device)
    B, K = idx.shape
    lv = fam.levels.validate(levels, K if fam.levels.by_rank else H, who) if fam.levels is not None else None
    b = _f32c(bias, "bias") if bias is not None else None
    if b is not None and tuple(b.shape) != (D,):
        raise ValueError(f"{who}: bias is {tuple(b.shape)}, expected [{D}]")
    recon = torch.empty((B, D) if lv is None else (len(lv), B, D), dtype=torch.float32, device=idx.device)
    below = torch.empty((len(lv), B), dtype=torch.int32, device=idx.device) if fam.below else None
    args = [_p(idx), _p(val)] + ([_p(counts)] if fam.ragged else []) + [B, K, _p(dictionary), H, D]
    args += ([n_bits] if kind == "binary" else []) + [float(mult), _p(b)]
    args += ([_bounds_arg(lv), len(lv)] if lv is not None else []) + [_p(recon)] + ([_p(below)] if fam.below else [])
    check(getattr(_lib.load(), f"{fam.symbol}_{kind}")(*args, _stream()))
    return (recon, below) if fam.below else recon


def _row_grad_lists(who: str, idx, counts, table, ragged: bool, need_2d: bool):
    """The lists and the table of a row gradient -> (idx, counts, table, B, K, H, D)."""
    if ragged:
        idx, _, counts = _batch_lists(who, idx, None, counts)
    else:
        _dev(idx, f"{who}: idx", torch.int32)
        if need_2d and idx.dim() != 2:
            raise ValueError(f"{who}: idx is {tuple(idx.shape)}, expected [B, K]")
        idx = idx.contiguous()
    table = _f32c(table, "table")
    B, K = idx.shape
    H, D = table.shape
    if ragged:
        _nested_D(who, D)
    else:
        _check_train_shape(D, K)
    return idx, counts, table, B, K, H, D


def _row_grad_latent(g_latent, W_enc, want_dx: bool, B: int, H: int, D: int):
    gL, gl_ld = _latent_grad(g_latent, B, H)
    W = _f32c(W_enc, "W_enc") if want_dx else None
    if W is not None and tuple(W.shape) != (H, D):
        raise ValueError(f"W_enc is {tuple(W.shape)}, expected [{H}, {D}]")
    return gL, gl_ld, W


def _row_grad_levels(fam: _RowGrad, who: str, idx, counts, table, step: float, grads, levels, g_latent, W_enc, want_dx: bool):
    """-> (G [L, B, D], gv [B, K], dx [B, D] or None) of the three level/point forms."""
    idx, counts, table, B, K, H, D = _row_grad_lists(who, idx, counts, table, fam.ragged, fam.need_2d)
    words = fam.levels
    lv = words.validate(levels, K if words.by_rank else H, who)
    grads = list(grads)
    if len(grads) != len(lv):
        raise ValueError(f"{who}: {len(grads)} {words.noun} gradients for {len(lv)} {words.noun}s")
    gs = []
    for l, g in enumerate(grads):
        if g is not None:
            g = _f32c(g, f"{words.grads}[{l}]")
            if tuple(g.shape) != (B, D) or g.device != idx.device:
                raise ValueError(f"{who}: {words.grads}[{l}] is {tuple(g.shape)} on {g.device}, expected [{B}, {D}] on {idx.device}")
        gs.append(g)
    gL, gl_ld, W = _row_grad_latent(g_latent, W_enc, want_dx, B, H, D)
    G = torch.empty((len(lv), B, D), dtype=torch.float32, device=idx.device)
    gv = torch.empty((B, K), dtype=torch.float32, device=idx.device)
    dx = torch.empty((B, D), dtype=torch.float32, device=idx.device) if want_dx else None
    garr = (C.c_void_p * len(gs))(*[0 if g is None else g.data_ptr() for g in gs])     # host array of device pointers
    args = [_p(idx)] + ([_p(counts)] if fam.ragged else [])
    check(getattr(_lib.load(), fam.symbol)(*args, B, K, _p(table), H, D, float(step), C.cast(garr, C.c_void_p), _bounds_arg(lv),
                                           len(lv), _p(gL), int(gl_ld), _p(W), _p(G), _p(gv), _p(dx), _stream()))
    return G, gv, dx


def _nested_G(who: str, G, L: int, B: int, D: int):
    if G is None:
        return None
    _dev(G, f"{who}: G", torch.float32)
    if tuple(G.shape) != (L, B, D) or not G.is_contiguous():
        raise ValueError(f"{who}: G is {tuple(G.shape)} (strides {G.stride()}), expected contiguous [{L}, {B}, {D}]")
    return G


def _unit_grad_levels(words: _Levels, who: str, offsets, entries, val, gv, x, G, levels, logits, n_bits: int, step: float,
                      g_polarize, want_encoder: bool, want_logits: bool):
    """The packed unit gradient with g_recon = G[level or point] -> (dW_enc, db_enc, dlogits)."""
    _dev(offsets, "offsets", torch.int32)
    _dev(entries, "entries", torch.int32)
    val, gv, x, logits = _f32c(val, "val"), _f32c(gv, "gv"), _f32c(x, "x"), _f32c(logits, "logits")
    if words.unit_prechecks and (val.dim() != 2 or x.dim() != 2 or offsets.dim() != 1):
        raise ValueError(f"{who}: val and x must be 2-D, offsets 1-D")
    B, k = val.shape
    D = x.shape[1]
    H = offsets.shape[0] - 1
    _check_train_shape(D, k)
    if (words.unit_prechecks and H < 1) or tuple(logits.shape) != (H, D * n_bits) or tuple(x.shape) != (B, D) \
            or tuple(gv.shape) != (B, k) or entries.numel() != B * k:
        raise ValueError(f"{who}: inconsistent shapes")
    if words.unit_prechecks and B * k >= 2 ** 31:
        raise ValueError(f"{who}: B * {words.k} = {B * k} is not below 2^31")
    lv = words.validate(levels, k if words.by_rank else H, who)
    G = _nested_G(who, G, len(lv), B, D)
    gP = _f32c(g_polarize.reshape(()), "g_polarize") if g_polarize is not None else None
    dev = x.device
    dW = torch.empty((H, D), dtype=torch.float32, device=dev) if want_encoder else None
    db = torch.empty((H,), dtype=torch.float32, device=dev) if want_encoder else None
    dl = torch.empty((H, D * n_bits), dtype=torch.float32, device=dev) if want_logits else None
    lib = _lib.load()
    symbol = words.unit_symbol.format("")
    ws = _train_ws(getattr(lib, symbol + "_workspace_bytes")(B, k, H, D), dev)
    check(getattr(lib, symbol)(_p(offsets.contiguous()), _p(entries.contiguous()), _p(val), _p(gv), B, k, _p(x), _p(G),
                               _bounds_arg(lv), len(lv), _p(logits), H, D, int(n_bits), float(step), _p(gP), _p(dW), _p(db),
                               _p(dl), _p(ws), ws.numel(), _stream()))
    return dW, db, dl


def _table_unit_grad_levels(words: _Levels, who: str, offsets, entries, val, gv, x, G, levels, want_encoder: bool,
                            want_decoder: bool):
    """The table unit gradient with g_recon = G[level or point] -> (dW_enc, db_enc, dW_dec)."""
    _dev(offsets, "offsets", torch.int32)
    _dev(entries, "entries", torch.int32)
    val, gv, x = _f32c(val, "val"), _f32c(gv, "gv"), _f32c(x, "x")
    if val.dim() != 2 or x.dim() != 2 or offsets.dim() != 1:
        raise ValueError(f"{who}: val and x must be 2-D, offsets 1-D")
    B, k = val.shape
    D = x.shape[1]
    H = offsets.shape[0] - 1
    _check_train_shape(D, k)
    if H < 1 or tuple(x.shape) != (B, D) or tuple(gv.shape) != (B, k) or entries.numel() != B * k:
        raise ValueError(f"{who}: inconsistent shapes")
    if B * k >= 2 ** 31:
        raise ValueError(f"{who}: B * {words.k} = {B * k} is not below 2^31")
    lv = words.validate(levels, k if words.by_rank else H, who)
    G = _nested_G(who, G, len(lv), B, D)
    dev = x.device
    dW = torch.empty((H, D), dtype=torch.float32, device=dev) if want_encoder else None
    db = torch.empty((H,), dtype=torch.float32, device=dev) if want_encoder else None
    dWd = torch.empty((D, H), dtype=torch.float32, device=dev) if want_decoder else None
    lib = _lib.load()
    symbol = words.unit_symbol.format("_table")
    ws = _train_ws(getattr(lib, symbol + "_workspace_bytes")(B, k, H, D), dev)
    check(getattr(lib, symbol)(_p(offsets.contiguous()), _p(entries.contiguous()), _p(val), _p(gv), B, k, _p(x), _p(G),
                               _bounds_arg(lv), len(lv), H, D, _p(dW), _p(db), _p(dWd), H, _p(ws), ws.numel(), _stream()))
    return dW, db, dWd


# ---- nested-dictionary (Matryoshka) objective of the top-k SAEs (include/qsae_nested.h, csrc/nested.hip) --------------------
@_on_tensor_device
def decode_nested_binary(idx, val, packed, D: int, n_bits: int, step: float, bias, bounds) -> torch.Tensor:
    """-> fp32 [L, B, D]: level l is decode_binary_sparse on the lists without the entries of units >= bounds[l], bit for bit,
    all levels from one walk over each row's list; see qsaen_decode_nested_binary."""
    return _decode_sparse(_DECODE_NESTED, "decode_nested_binary", idx, val, None, packed, D, n_bits, step, bias, bounds)


@_on_tensor_device
def decode_nested_table(idx, val, table: torch.Tensor, scale: float, bias, bounds) -> torch.Tensor:
    """-> fp32 [L, B, D]: level l is decode_table_sparse on the lists without the entries of units >= bounds[l], bit for bit;
    see qsaen_decode_nested_table."""
    return _decode_sparse(_DECODE_NESTED, "decode_nested_table", idx, val, None, table, None, None, scale, bias, bounds)


@_on_tensor_device
def train_row_grad_nested(idx: torch.Tensor, table: torch.Tensor, step: float, g_levels, bounds,
                          g_latent: Optional[torch.Tensor], W_enc: Optional[torch.Tensor], want_dx: bool = False):
    """-> (G fp32 [L, B, D], gv fp32 [B, k], dx fp32 [B, D] or None).  ``g_levels``: L gradients [B, D], None for a level the
    loss does not read.  G holds their suffix sums; gv and dx are train_row_grad's with g_recon = G[level(unit)] per entry.  See
    qsaen_row_grad_nested."""
    return _row_grad_levels(_ROW_NESTED, "train_row_grad_nested", idx, None, table, step, g_levels, bounds, g_latent, W_enc,
                            want_dx)


@_on_tensor_device
def train_unit_grad_nested(offsets: torch.Tensor, entries: torch.Tensor, val: torch.Tensor, gv: torch.Tensor, x: torch.Tensor,
                           G: Optional[torch.Tensor], bounds, logits: torch.Tensor, n_bits: int, step: float,
                           g_polarize: Optional[torch.Tensor], want_encoder: bool = True, want_logits: bool = True):
    """train_unit_grad with g_recon = G[level(h)] for unit h (G fp32 [L, B, D] from train_row_grad_nested, or None);
    see qsaen_train_unit_grad_nested."""
    return _unit_grad_levels(_NESTED, "train_unit_grad_nested", offsets, entries, val, gv, x, G, bounds, logits, n_bits, step,
                             g_polarize, want_encoder, want_logits)


@_on_tensor_device
def train_table_unit_grad_nested(offsets: torch.Tensor, entries: torch.Tensor, val: torch.Tensor, gv: torch.Tensor,
                                 x: torch.Tensor, G: Optional[torch.Tensor], bounds, want_encoder: bool = True,
                                 want_decoder: bool = True):
    """train_table_unit_grad with g_recon = G[level(h)] for unit h; see qsaen_train_table_unit_grad_nested."""
    return _table_unit_grad_levels(_NESTED, "train_table_unit_grad_nested", offsets, entries, val, gv, x, G, bounds, want_encoder,
                                   want_decoder)


# ---- Multi-TopK objective of the top-k SAEs (include/qsae_multik.h, csrc/multi_topk.hip) ------------------------------------
@_on_tensor_device
def decode_multik_binary(idx, val, packed, D: int, n_bits: int, step: float, bias, ks) -> torch.Tensor:
    """-> fp32 [P, B, D]: point p is decode_binary_sparse on idx[:, :ks[p]], val[:, :ks[p]], bit for bit, every dictionary row
    gathered once for up to four points; see qsaek_decode_multik_binary."""
    return _decode_sparse(_DECODE_MULTIK, "decode_multik_binary", idx, val, None, packed, D, n_bits, step, bias, ks)


@_on_tensor_device
def decode_multik_table(idx, val, table: torch.Tensor, scale: float, bias, ks) -> torch.Tensor:
    """-> fp32 [P, B, D]: point p is decode_table_sparse on idx[:, :ks[p]], val[:, :ks[p]], bit for bit; see
    qsaek_decode_multik_table."""
    return _decode_sparse(_DECODE_MULTIK, "decode_multik_table", idx, val, None, table, None, None, scale, bias, ks)


@_on_tensor_device
def train_row_grad_multik(idx: torch.Tensor, table: torch.Tensor, step: float, g_points, ks,
                          g_latent: Optional[torch.Tensor], W_enc: Optional[torch.Tensor], want_dx: bool = False):
    """-> (G fp32 [P, B, D], gv fp32 [B, K], dx fp32 [B, D] or None).  ``g_points``: P gradients [B, D], None for a point the
    loss does not read.  G holds their suffix sums; gv and dx are train_row_grad's with g_recon = G[point(rank)] per entry.  See
    qsaek_row_grad_multik."""
    return _row_grad_levels(_ROW_MULTIK, "train_row_grad_multik", idx, None, table, step, g_points, ks, g_latent, W_enc, want_dx)


@_on_tensor_device
def train_unit_grad_multik(offsets: torch.Tensor, entries: torch.Tensor, val: torch.Tensor, gv: torch.Tensor, x: torch.Tensor,
                           G: Optional[torch.Tensor], ks, logits: torch.Tensor, n_bits: int, step: float,
                           g_polarize: Optional[torch.Tensor], want_encoder: bool = True, want_logits: bool = True):
    """train_unit_grad with g_recon = G[point(e % K)] for list entry e (G fp32 [P, B, D] from train_row_grad_multik, or None);
    see qsaek_train_unit_grad_multik."""
    return _unit_grad_levels(_MULTIK, "train_unit_grad_multik", offsets, entries, val, gv, x, G, ks, logits, n_bits, step,
                             g_polarize, want_encoder, want_logits)


@_on_tensor_device
def train_table_unit_grad_multik(offsets: torch.Tensor, entries: torch.Tensor, val: torch.Tensor, gv: torch.Tensor,
                                 x: torch.Tensor, G: Optional[torch.Tensor], ks, want_encoder: bool = True,
                                 want_decoder: bool = True):
    """train_table_unit_grad with g_recon = G[point(e % K)] for list entry e; see qsaek_train_table_unit_grad_multik."""
    return _table_unit_grad_levels(_MULTIK, "train_table_unit_grad_multik", offsets, entries, val, gv, x, G, ks, want_encoder,
                                   want_decoder)


# ---- BatchTopK of the top-k SAEs (include/qsae_batch.h, csrc/batch_topk.hip, csrc/batch_topk_decode.hip) -------------------
BATCH_TOPK_MAX_K = 256
BATCH_TOPK_REPORT_WORDS = 4       # selected, saturated rows, empty rows, bits of the smallest selected value


def _batch_vals(who: str, val):
    _dev(val, f"{who}: val", torch.float32)
    if val.dim() != 2 or val.shape[1] < 1:
        raise ValueError(f"{who}: val is {tuple(val.shape)}, expected [B, K] with K >= 1")
    if val.shape[1] > BATCH_TOPK_MAX_K:
        raise ValueError(f"{who}: the cap K = {val.shape[1]} exceeds {BATCH_TOPK_MAX_K}")
    if val.shape[0] * val.shape[1] >= 2 ** 31:
        raise ValueError(f"{who}: B * K = {val.shape[0] * val.shape[1]} is not below 2^31")
    return val.contiguous()


def _batch_lists(who: str, idx, val, counts):
    _dev(idx, f"{who}: idx", torch.int32)
    _dev(counts, f"{who}: counts", torch.int32)
    if val is not None:
        val = _batch_vals(who, val)
        if idx.shape != val.shape or idx.device != val.device:
            raise ValueError(f"{who}: idx is {tuple(idx.shape)}, val {tuple(val.shape)}; expected two [B, K] tensors on one device")
    if idx.dim() != 2 or not 1 <= idx.shape[1] <= BATCH_TOPK_MAX_K:
        raise ValueError(f"{who}: idx is {tuple(idx.shape)}, expected [B, K] with 1 <= K <= {BATCH_TOPK_MAX_K}")
    if tuple(counts.shape) != (idx.shape[0],) or counts.device != idx.device:
        raise ValueError(f"{who}: counts is {tuple(counts.shape)} on {counts.device}, expected [{idx.shape[0]}] on {idx.device}")
    return idx.contiguous(), val, counts.contiguous()


def _batch_state(who: str, theta, batches, device):
    if (theta is None) != (batches is None):
        raise ValueError(f"{who}: theta and batches go together")
    if theta is None:
        return
    _dev(theta, f"{who}: theta", torch.float32)
    _dev(batches, f"{who}: batches", torch.int64)
    if theta.numel() != 1 or batches.numel() != 1 or theta.device != device or batches.device != device:
        raise ValueError(f"{who}: theta and batches are one element each on {device}")


@_on_tensor_device
def batch_select(val: torch.Tensor, n_select: int, want_val: bool = True, theta: Optional[torch.Tensor] = None,
                 batches: Optional[torch.Tensor] = None, lr: float = 0.01):
    """The n_select largest entries of the whole batch of top-K lists ``val`` [B, K] (ties to the lowest row, then position)
    -> (counts int32 [B], val_sel fp32 [B, K] or None, report int64 [4]); updates the threshold state (theta fp32, batches
    int64, one element each, in place) when given.  No host read.  See qsaeb_batch_select."""
    who = "batch_select"
    val = _batch_vals(who, val)
    B, K = val.shape
    n_select = int(n_select)
    if not 0 <= n_select <= B * K:
        raise ValueError(f"{who}: n_select = {n_select} is outside 0 .. B * K = {B * K}")
    _batch_state(who, theta, batches, val.device)
    counts = torch.empty((B,), dtype=torch.int32, device=val.device)
    val_sel = torch.empty_like(val) if want_val else None
    report = torch.zeros((BATCH_TOPK_REPORT_WORDS,), dtype=torch.int64, device=val.device)
    lib = _lib.load()
    ws = _train_ws(lib.qsaeb_batch_select_workspace_bytes(B, K), val.device)
    check(lib.qsaeb_batch_select(_p(val), B, K, n_select, _p(counts), _p(val_sel), _p(report), _p(theta), _p(batches), float(lr),
                                 _p(ws), ws.numel(), _stream()))
    return counts, val_sel, report


@_on_tensor_device
def threshold_select(val: torch.Tensor, theta, want_val: bool = True):
    """counts[r] = the longest prefix of row r of ``val`` [B, K] with val >= theta (a float compare; ``theta``: a one-element
    fp32 device tensor, read on the device, or a number) -> (counts, val_sel or None, report) as batch_select.  See
    qsaeb_threshold_select."""
    who = "threshold_select"
    val = _batch_vals(who, val)
    B, K = val.shape
    if isinstance(theta, torch.Tensor):
        _dev(theta, f"{who}: theta", torch.float32)
        if theta.numel() != 1 or theta.device != val.device:
            raise ValueError(f"{who}: theta is one element on {val.device}")
        t_dev, t_host = theta, 0.0
    else:
        t_dev, t_host = None, float(theta)
    counts = torch.empty((B,), dtype=torch.int32, device=val.device)
    val_sel = torch.empty_like(val) if want_val else None
    report = torch.zeros((BATCH_TOPK_REPORT_WORDS,), dtype=torch.int64, device=val.device)
    lib = _lib.load()
    ws = _train_ws(lib.qsaeb_threshold_select_workspace_bytes(B, K), val.device)
    check(lib.qsaeb_threshold_select(_p(val), B, K, _p(t_dev), t_host, _p(counts), _p(val_sel), _p(report), _p(ws), ws.numel(),
                                     _stream()))
    return counts, val_sel, report


@_on_tensor_device
def decode_ragged_binary(idx, val, counts, packed, D: int, n_bits: int, step: float, bias=None) -> torch.Tensor:
    """-> fp32 [B, D]: row r is decode_binary_sparse on the first counts[r] entries of its list, bit for bit; an entry behind
    the prefix is not read.  See qsaeb_decode_ragged_binary."""
    return _decode_sparse(_DECODE_RAGGED, "decode_ragged_binary", idx, val, counts, packed, D, n_bits, step, bias, None)


@_on_tensor_device
def decode_ragged_table(idx, val, counts, table: torch.Tensor, scale: float = 1.0, bias=None) -> torch.Tensor:
    """-> fp32 [B, D]: row r is decode_table_sparse on the first counts[r] entries of its list, bit for bit.  See
    qsaeb_decode_ragged_table."""
    return _decode_sparse(_DECODE_RAGGED, "decode_ragged_table", idx, val, counts, table, None, None, scale, bias, None)


@_on_tensor_device
def train_row_grad_ragged(idx: torch.Tensor, counts: torch.Tensor, table: torch.Tensor, step: float,
                          g_recon: Optional[torch.Tensor], g_latent: Optional[torch.Tensor],
                          W_enc: Optional[torch.Tensor] = None, want_dx: bool = False):
    """-> (gv fp32 [B, K], dx fp32 [B, D] or None): train_row_grad on the first counts[r] entries of every row, bit for bit;
    gv behind the prefix is +0.  See qsaeb_row_grad_ragged."""
    who = "train_row_grad_ragged"
    idx, counts, table, B, K, H, D = _row_grad_lists(who, idx, counts, table, True, False)
    gR = _f32c(g_recon, "g_recon") if g_recon is not None else None
    if gR is not None and tuple(gR.shape) != (B, D):
        raise ValueError(f"g_recon is {tuple(gR.shape)}, expected [{B}, {D}]")
    gL, gl_ld, W = _row_grad_latent(g_latent, W_enc, want_dx, B, H, D)
    gv = torch.empty((B, K), dtype=torch.float32, device=idx.device)
    dx = torch.empty((B, D), dtype=torch.float32, device=idx.device) if want_dx else None
    check(_lib.load().qsaeb_row_grad_ragged(_p(idx), _p(counts), B, K, _p(table), H, D, float(step), _p(gR), _p(gL), int(gl_ld),
                                            _p(W), _p(gv), _p(dx), _stream()))
    return gv, dx


@_on_tensor_device
def train_csr_ragged(idx: torch.Tensor, counts: torch.Tensor, H: int):
    """The first counts[r] entries of the lists [B, K] grouped by unit -> (offsets int32 [H + 1], entries int32 [B K], of which
    the first offsets[H] are set and the rest are -1): what train_unit_grad / train_table_unit_grad take together with
    [B, K] val_sel and gv.  See qsaeb_csr_ragged."""
    who = "train_csr_ragged"
    idx, _, counts = _batch_lists(who, idx, None, counts)
    B, K = idx.shape
    H = int(H)
    if H < 1:
        raise ValueError(f"{who}: H = {H} must be positive")
    offsets = torch.empty((H + 1,), dtype=torch.int32, device=idx.device)
    entries = torch.empty((B * K,), dtype=torch.int32, device=idx.device)
    lib = _lib.load()
    ws = _train_ws(lib.qsaeb_csr_ragged_workspace_bytes(B, K, H), idx.device)
    check(lib.qsaeb_csr_ragged(_p(idx), _p(counts), B, K, H, _p(offsets), _p(entries), _p(ws), ws.numel(), _stream()))
    return offsets, entries


# ---- nested levels over the ragged rows of BatchTopK (include/qsae_nested_batch.h, csrc/nested_ragged.hip) ------------------
@_on_tensor_device
def decode_nested_ragged_binary(idx, val, counts, packed, D: int, n_bits: int, step: float, bias, bounds):
    """-> (levels fp32 [L, B, D], counts_below int32 [L, B]): level l of row r is decode_nested_binary on the first counts[r]
    entries of its list, bit for bit; counts_below[l, r] = its kept entries below bounds[l].  An entry behind the prefix is not
    read.  See qsaem_decode_nested_ragged_binary."""
    return _decode_sparse(_DECODE_NESTED_RAGGED, "decode_nested_ragged_binary", idx, val, counts, packed, D, n_bits, step, bias,
                          bounds)


@_on_tensor_device
def decode_nested_ragged_table(idx, val, counts, table: torch.Tensor, scale: float, bias, bounds):
    """-> (levels fp32 [L, B, D], counts_below int32 [L, B]): level l of row r is decode_nested_table on the first counts[r]
    entries of its list, bit for bit.  See qsaem_decode_nested_ragged_table."""
    return _decode_sparse(_DECODE_NESTED_RAGGED, "decode_nested_ragged_table", idx, val, counts, table, None, None, scale, bias,
                          bounds)


@_on_tensor_device
def train_row_grad_nested_ragged(idx: torch.Tensor, counts: torch.Tensor, table: torch.Tensor, step: float, g_levels, bounds,
                                 g_latent: Optional[torch.Tensor], W_enc: Optional[torch.Tensor] = None, want_dx: bool = False):
    """-> (G fp32 [L, B, D], gv fp32 [B, K], dx fp32 [B, D] or None): train_row_grad_nested on the first counts[r] entries of
    every row, bit for bit; G is written for every row, gv behind the prefix is +0.  See qsaem_row_grad_nested_ragged."""
    return _row_grad_levels(_ROW_NESTED_RAGGED, "train_row_grad_nested_ragged", idx, counts, table, step, g_levels, bounds,
                            g_latent, W_enc, want_dx)


# ---- JumpReLU of the top-k SAEs (include/qsae_jump.h, csrc/jumprelu.hip) ------------------------------------------------------
JUMP_MAX_K = 256
JUMP_REPORT_WORDS = 6             # selected, band entries, saturated rows, empty rows, uncertified rows, bits of theta_min


def jump_half_eps(eps: float) -> float:
    """fl32(0.5f * fl32(eps)), the half bandwidth the kernels compare against (one rounding: the product is exact in fp64)"""
    return C.c_float(0.5 * C.c_float(float(eps)).value).value


def _jump_eps(who: str, eps) -> float:
    eps = C.c_float(float(eps)).value
    if not (eps > 0.0 and eps != float("inf")):
        raise ValueError(f"{who}: the bandwidth eps = {eps} must be positive and finite in fp32")
    return eps


def _jump_theta(who: str, theta, device) -> torch.Tensor:
    _dev(theta, f"{who}: theta", torch.float32)
    if theta.dim() != 1 or theta.shape[0] < 1 or theta.device != device:
        raise ValueError(f"{who}: theta is {tuple(theta.shape)} on {theta.device}, expected [H] with H >= 1 on {device}")
    return theta.contiguous()


@_on_tensor_device
def jump_select(idx: torch.Tensor, val: torch.Tensor, theta: torch.Tensor, eps: float, want_band: bool = True):
    """JumpReLU on the top-K lists (idx int32, val fp32, both [B, K]) with the per-unit thresholds ``theta`` fp32 [H]: an entry
    is selected iff val > theta[idx], in the band iff |val - theta[idx]| < eps / 2 -> (idx_sel, val_sel, counts, idx_band or
    None, counts_band or None, l0 fp32 [1], report int64 [6]): the stable partition of every row by either predicate, the mean
    number of selected entries per row, and {selected, band entries, saturated rows, empty rows, uncertified rows, bits of the
    smallest threshold}.  No host read.  See qsaej_jump_select."""
    who = "jump_select"
    _dev(idx, f"{who}: idx", torch.int32)
    val = _batch_vals(who, val)
    if idx.shape != val.shape or idx.device != val.device:
        raise ValueError(f"{who}: idx is {tuple(idx.shape)}, val {tuple(val.shape)}; expected two [B, K] tensors on one device")
    idx = idx.contiguous()
    theta = _jump_theta(who, theta, val.device)
    eps = _jump_eps(who, eps)
    B, K = val.shape
    H = theta.shape[0]
    dev = val.device
    idx_sel, val_sel = torch.empty_like(idx), torch.empty_like(val)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    idx_band = torch.empty_like(idx) if want_band else None
    counts_band = torch.empty((B,), dtype=torch.int32, device=dev) if want_band else None
    l0 = torch.zeros((1,), dtype=torch.float32, device=dev)
    report = torch.zeros((JUMP_REPORT_WORDS,), dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = _train_ws(lib.qsaej_jump_select_workspace_bytes(B, K, H), dev)
    check(lib.qsaej_jump_select(_p(idx), _p(val), B, K, _p(theta), H, eps, jump_half_eps(eps), _p(idx_sel), _p(val_sel), _p(counts),
                                _p(idx_band), _p(counts_band), _p(l0), _p(report), _p(ws), ws.numel(), _stream()))
    return idx_sel, val_sel, counts, idx_band, counts_band, l0, report


@_on_tensor_device
def jump_threshold_grad(offsets: torch.Tensor, entries: torch.Tensor, gv_band: Optional[torch.Tensor], theta: torch.Tensor,
                        g_l0: Optional[torch.Tensor], B: int, K: int, eps: float) -> torch.Tensor:
    """-> dtheta fp32 [H]: for every unit, -(theta[h] * sum of gv_band over its band entries + g_l0 * n / B) / eps in fp64 with
    one rounding, from the lists train_csr_ragged writes over (idx_band, counts_band) and the gv train_row_grad_ragged writes
    over them (None: no reconstruction term); g_l0: the gradient that reached l0 (one fp32 element on the device) or None.
    See qsaej_threshold_grad."""
    who = "jump_threshold_grad"
    _dev(offsets, f"{who}: offsets", torch.int32)
    _dev(entries, f"{who}: entries", torch.int32)
    theta = _jump_theta(who, theta, offsets.device)
    eps = _jump_eps(who, eps)
    B, K, H = int(B), int(K), theta.shape[0]
    if B < 0 or not 1 <= K <= JUMP_MAX_K or B * K >= 2 ** 31:
        raise ValueError(f"{who}: B = {B}, K = {K}; expected B >= 0, 1 <= K <= {JUMP_MAX_K} and B * K below 2^31")
    if tuple(offsets.shape) != (H + 1,) or entries.dim() != 1 or entries.shape[0] < B * K or entries.device != offsets.device:
        raise ValueError(f"{who}: offsets is {tuple(offsets.shape)}, entries {tuple(entries.shape)}; expected [{H + 1}] and "
                         f"[{B * K}] on one device")
    if gv_band is not None:
        gv_band = _f32c(gv_band, f"{who}: gv_band")
        if gv_band.numel() != B * K or gv_band.device != offsets.device:
            raise ValueError(f"{who}: gv_band is {tuple(gv_band.shape)} on {gv_band.device}, expected [{B}, {K}] on {offsets.device}")
    if g_l0 is not None:
        g_l0 = _f32c(g_l0, f"{who}: g_l0")
        if g_l0.numel() != 1 or g_l0.device != offsets.device:
            raise ValueError(f"{who}: g_l0 is one element on {offsets.device}")
    dtheta = torch.empty((H,), dtype=torch.float32, device=offsets.device)
    check(_lib.load().qsaej_threshold_grad(_p(offsets.contiguous()), _p(entries.contiguous()), _p(gv_band), _p(theta), _p(g_l0), B, K,
                                           H, eps, _p(dtheta), _stream()))
    return dtheta


# ---- the dense (uncapped) JumpReLU encoder (include/qsae_jump_dense.h, csrc/jump_dense.hip) -----------------------------------
JUMP_DENSE_MAX_K = 256
JUMP_DENSE_REPORT_WORDS = 6       # selected, band entries, truncated rows, empty rows, band-truncated rows, firing units (uncapped)


@_on_tensor_device
def encode_jump(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], theta: torch.Tensor, K: int, bandwidth: float,
                want_band: bool = True):
    """JumpReLU over ALL pre-activations z = x W^T + bias (the encoder's fp32 fmaf chain; x fp32 [B, D], W fp32 [H, D], bias fp32
    [H] or None) with the per-unit thresholds ``theta`` fp32 [H]: unit h fires in row r iff z > theta[h], is in the band iff
    |z - theta[h]| < bandwidth / 2 -> (idx_sel, val_sel, counts, idx_band or None, counts_band or None, l0 fp32 [1], report
    int64 [6]), in the order ``jump_select`` returns: the firing units of every row by value descending, then unit ascending,
    the first ``K`` of them (-1 / +0 behind the first counts[r]), the same for the band, the mean number of firing units per
    row from the uncapped counts, and {selected, band entries, truncated rows, empty rows, band-truncated rows, firing units}.
    No top-K list, no certificate, no host read.  See qsaed_encode_jump."""
    who = "encode_jump"
    x, W = _f32c(x, f"{who}: x"), _f32c(W, f"{who}: W")
    if x.dim() != 2 or W.dim() != 2 or x.shape[1] != W.shape[1] or W.shape[0] < 1 or W.device != x.device:
        raise ValueError(f"{who}: x is {tuple(x.shape)} on {x.device}, W {tuple(W.shape)} on {W.device}; expected [B, D] and [H, D] "
                         f"on one device")
    B, D = x.shape
    H = W.shape[0]
    b = _f32c(bias, f"{who}: bias") if bias is not None else None
    if b is not None and (tuple(b.shape) != (H,) or b.device != x.device):
        raise ValueError(f"{who}: bias is {tuple(b.shape)} on {b.device}, expected [{H}] on {x.device}")
    theta = _jump_theta(who, theta, x.device)
    if theta.shape[0] != H:
        raise ValueError(f"{who}: theta is {tuple(theta.shape)}, expected [{H}]")
    eps = _jump_eps(who, bandwidth)
    K = int(K)
    if not 1 <= K <= min(JUMP_DENSE_MAX_K, H):
        raise ValueError(f"{who}: K = {K} is outside 1 .. {min(JUMP_DENSE_MAX_K, H)} (the width of the kernel's lists and H = {H})")
    if D < 4 or D % 4 != 0:
        raise ValueError(f"{who}: D = {D} must be a positive multiple of 4")
    if B * K >= 2 ** 31:
        raise ValueError(f"{who}: B * K = {B * K} is not below 2^31")
    dev = x.device
    idx_sel = torch.empty((B, K), dtype=torch.int32, device=dev)
    val_sel = torch.empty((B, K), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    idx_band = torch.empty((B, K), dtype=torch.int32, device=dev) if want_band else None
    counts_band = torch.empty((B,), dtype=torch.int32, device=dev) if want_band else None
    l0 = torch.zeros((1,), dtype=torch.float32, device=dev)
    report = torch.zeros((JUMP_DENSE_REPORT_WORDS,), dtype=torch.int64, device=dev)
    if B == 0:
        return idx_sel, val_sel, counts, idx_band, counts_band, l0, report
    lib = _lib.load()
    ws = _train_ws(lib.qsaed_encode_jump_workspace_bytes(B, D, H, K), dev)
    check(lib.qsaed_encode_jump(_p(x), D, _p(W), D, _p(b), _p(theta), B, D, H, K, eps, jump_half_eps(eps), _p(idx_sel), _p(val_sel),
                                _p(counts), _p(idx_band), _p(counts_band), _p(l0), _p(report), _p(ws), ws.numel(), _stream()))
    return idx_sel, val_sel, counts, idx_band, counts_band, l0, report


# ---- the dense BatchTopK encoder (include/qsae_batch_dense.h, csrc/batch_dense.hip) ------------------------------------------
BATCH_DENSE_MAX_K = 256
BATCH_DENSE_REPORT_WORDS = 8      # selected, saturated rows, empty rows, bits of the smallest selected value, candidates of attempt
#                                   one, second attempt ran, rows with more than K candidates, bits of the floor used


@_on_tensor_device
def encode_batch_topk(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], n_select: int, K: int, floor,
                      floor_ratio: float = 1.0, state=None):
    """BatchTopK capped at ``K`` per row straight from the encoder: the ``n_select`` largest entries of the whole batch of top-K
    lists of z = x W^T + bias (the encoder's fp32 fmaf chain; x fp32 [B, D], W fp32 [H, D], bias fp32 [H] or None), ties to the
    lowest row, then list position -> (idx_sel int32 [B, K], val_sel fp32 [B, K], counts int32 [B], report int64 [8]): what
    ``batch_select`` gives on the lists of ``encode_topk`` at width K, with -1 / +0 behind the first counts[r] entries of a row.
    ``floor``: only pre-activations above it are candidates; a one-element fp32 device tensor (read on the device, and
    overwritten with fl32(floor_ratio * m), m the batch's smallest selected value, when something was selected and m > 0) or a
    number.  The result does not depend on it: when fewer than n_select candidates lie above it a second attempt without a floor
    runs on the device (report[5]).  ``state``: None or (theta fp32 [1], batches int64 [1], lr), the threshold state of
    ``batch_select``, updated in place.  No host read.  See qsaebd_encode_batch_topk."""
    who = "encode_batch_topk"
    x, W = _f32c(x, f"{who}: x"), _f32c(W, f"{who}: W")
    if x.dim() != 2 or W.dim() != 2 or x.shape[1] != W.shape[1] or W.shape[0] < 1 or W.device != x.device:
        raise ValueError(f"{who}: x is {tuple(x.shape)} on {x.device}, W {tuple(W.shape)} on {W.device}; expected [B, D] and [H, D] "
                         f"on one device")
    B, D = x.shape
    H = W.shape[0]
    b = _f32c(bias, f"{who}: bias") if bias is not None else None
    if b is not None and (tuple(b.shape) != (H,) or b.device != x.device):
        raise ValueError(f"{who}: bias is {tuple(b.shape)} on {b.device}, expected [{H}] on {x.device}")
    K = int(K)
    if not 1 <= K <= min(BATCH_DENSE_MAX_K, H):
        raise ValueError(f"{who}: K = {K} is outside 1 .. {min(BATCH_DENSE_MAX_K, H)} (the width of the kernel's lists and H = {H})")
    if D < 4 or D % 4 != 0:
        raise ValueError(f"{who}: D = {D} must be a positive multiple of 4")
    if B * K >= 2 ** 31:
        raise ValueError(f"{who}: B * K = {B * K} is not below 2^31")
    n_select = int(n_select)
    if not 0 <= n_select <= B * K:
        raise ValueError(f"{who}: n_select = {n_select} is outside 0 .. B * K = {B * K}")
    floor_ratio = float(floor_ratio)
    if not 0.0 < floor_ratio <= 1.0:
        raise ValueError(f"{who}: floor_ratio = {floor_ratio} is outside (0, 1]")
    if isinstance(floor, torch.Tensor):
        _dev(floor, f"{who}: floor", torch.float32)
        if floor.numel() != 1 or floor.device != x.device or not floor.is_contiguous():
            raise ValueError(f"{who}: floor is one element on {x.device}")
        f_dev, f_host = floor, 0.0
    else:
        f_dev, f_host = None, float(floor)
    theta, batches, lr = state if state is not None else (None, None, 0.0)
    _batch_state(who, theta, batches, x.device)
    dev = x.device
    idx_sel = torch.empty((B, K), dtype=torch.int32, device=dev)
    val_sel = torch.empty((B, K), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    report = torch.zeros((BATCH_DENSE_REPORT_WORDS,), dtype=torch.int64, device=dev)
    if B == 0:
        return idx_sel, val_sel, counts, report
    lib = _lib.load()
    ws = _train_ws(lib.qsaebd_encode_batch_topk_workspace_bytes(B, D, H, K), dev)
    check(lib.qsaebd_encode_batch_topk(_p(x), D, _p(W), D, _p(b), B, D, H, K, n_select, _p(f_dev), f_host, floor_ratio, _p(idx_sel),
                                       _p(val_sel), _p(counts), _p(report), _p(theta), _p(batches), float(lr), _p(ws), ws.numel(),
                                       _stream()))
    return idx_sel, val_sel, counts, report


# ---- dictionaries wider than one selection kernel: top-k over hidden slabs (include/qsae_wide.h, csrc/wide.hip) ------------------
WIDE_MAX_SLABS = 32
WIDE_MAX_H = 1 << 20
WIDE_DEFAULT_SLAB = 32768


def wide_plan(H: int, k: int, slab: int = WIDE_DEFAULT_SLAB):
    """-> the S + 1 slab starts of qsaew_slab_plan (ascending multiples of 256, the last entry H); ValueError where it refuses."""
    starts = (C.c_int * (WIDE_MAX_SLABS + 1))()
    lib = _lib.load()
    S = int(lib.qsaew_slab_plan(int(H), int(k), int(slab), starts))
    if S < 1:
        msg = lib.qsae_last_error()
        raise ValueError(f"wide_plan: H = {H}, k = {k}, slab = {slab}: {msg.decode(errors='replace') if msg else S}")
    return [int(starts[s]) for s in range(S + 1)]


def encode_topk_wide_supported(B: int, D: int, H: int, k: int, slab: int = WIDE_DEFAULT_SLAB) -> bool:
    """Whether encode_topk_wide runs this shape: H <= 2^20 in at most 32 slabs of at least k units, each a shape that some
    existing selection form takes."""
    return int(_lib.load().qsaew_encode_topk_prefilter_workspace_bytes(int(B), int(D), int(H), int(k), int(slab))) > 0


@_on_tensor_device
def merge_topk_parts(pidx: torch.Tensor, pval: torch.Tensor, starts, dense: Optional[torch.Tensor] = None):
    """The rows' top-k from the top-k lists of S hidden slabs: ``pidx`` int32 / ``pval`` fp32 [S, B, k], each list by value
    descending, then unit ascending, unit ids relative to ``starts[s]`` (``starts``: S + 1 ascending ints, ``wide_plan``)
    -> (idx int32 [B, k] with global unit ids, val fp32 [B, k]) in the same order, the order of the one-piece kernels.  ``dense``
    (fp32 [B, >= starts[S]], unit column stride): +0 is stored at the element of every entry that lost.  See qsaew_merge_topk."""
    who = "merge_topk_parts"
    _dev(pidx, f"{who}: pidx", torch.int32)
    _dev(pval, f"{who}: pval", torch.float32)
    if pidx.dim() != 3 or pidx.shape != pval.shape or pidx.device != pval.device:
        raise ValueError(f"{who}: pidx is {tuple(pidx.shape)}, pval {tuple(pval.shape)}; expected [S, B, k] twice on one device")
    S, B, k = (int(n) for n in pidx.shape)
    starts = [int(h) for h in starts]
    if not 1 <= S <= WIDE_MAX_SLABS or len(starts) != S + 1 or k < 1:
        raise ValueError(f"{who}: S = {S}, k = {k}, {len(starts)} starts; expected 1 <= S <= {WIDE_MAX_SLABS}, k >= 1 and S + 1 starts")
    if starts[0] < 0 or any(starts[s + 1] - starts[s] < k for s in range(S)):
        raise ValueError(f"{who}: starts = {starts}: every slab must be at least k = {k} wide")
    if B * k >= 2 ** 31:
        raise ValueError(f"{who}: B * k = {B * k} is not below 2^31")
    pidx, pval = pidx.contiguous(), pval.contiguous()
    ld = 0
    if dense is not None:
        _dev(dense, f"{who}: dense", torch.float32)
        if dense.dim() != 2 or dense.shape[0] != B or dense.shape[1] < starts[S] or (B and dense.stride(1) != 1) \
                or dense.device != pidx.device:
            raise ValueError(f"{who}: dense is {tuple(dense.shape)}; expected [{B}, >= {starts[S]}] with unit column stride")
        ld = dense.stride(0) if B else starts[S]
        _latent_pool_forget(dense)
    idx = torch.empty((B, k), dtype=torch.int32, device=pidx.device)
    val = torch.empty((B, k), dtype=torch.float32, device=pidx.device)
    check(_lib.load().qsaew_merge_topk(_p(pidx), _p(pval), S, B, k, (C.c_int * (S + 1))(*starts), _p(idx), _p(val), _p(dense), ld,
                                       _stream()))
    return idx, val


@_on_tensor_device
def encode_topk_wide(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], k: int, *, Wq: Optional[torch.Tensor] = None,
                     meta: Optional[torch.Tensor] = None, want_dense: bool = True, slab: int = WIDE_DEFAULT_SLAB,
                     spec_rows: int = 0, info: Optional[dict] = None):
    """Encoder + exact per-row top-k (+ dense latent) over a dictionary of up to 2^20 units: the hidden range in slabs of
    ``wide_plan(H, k, slab)``, every slab through the existing selection forms on its row range of ``W`` (nothing is copied), the
    slabs' lists merged on the device -> (idx int32 [B, k], val fp32 [B, k], dense [B, H] or None), bit for bit what
    ``encode_topk_latent`` gives wherever that runs.  With ``Wq`` and ``meta`` (``prefilter_pack_w`` of the WHOLE matrix) a slab
    the fp16 prefilter takes goes through it; without, every slab takes the exact fused or chunked form.  ``info`` receives
    ``flagged_rows`` (summed over the slabs) and ``slabs``.  See qsaew_encode_topk / qsaew_encode_topk_prefilter."""
    who = "encode_topk_wide"
    x, W = _f32c(x, f"{who}: x"), _f32c(W, f"{who}: W")
    if x.dim() != 2 or W.dim() != 2 or x.shape[1] != W.shape[1] or W.device != x.device:
        raise ValueError(f"{who}: x is {tuple(x.shape)} on {x.device}, W {tuple(W.shape)} on {W.device}; expected [B, D] and [H, D] "
                         f"on one device")
    B, D = x.shape
    H = W.shape[0]
    k, slab = int(k), int(slab)
    b = _f32c(bias, f"{who}: bias") if bias is not None else None
    if b is not None and (tuple(b.shape) != (H,) or b.device != x.device):
        raise ValueError(f"{who}: bias is {tuple(b.shape)} on {b.device}, expected [{H}] on {x.device}")
    if (Wq is None) != (meta is None):
        raise ValueError(f"{who}: Wq and meta come together (prefilter_pack_w of the whole matrix)")
    starts = wide_plan(H, k, slab)
    pref = Wq is not None
    if pref:
        _dev(Wq, f"{who}: Wq", torch.float16)
        _dev(meta, f"{who}: meta", torch.float32)
        if tuple(Wq.shape) != (H, D) or not Wq.is_contiguous() or meta.numel() != 4 or Wq.device != x.device or meta.device != x.device:
            raise ValueError(f"{who}: Wq is {tuple(Wq.shape)}, meta {tuple(meta.shape)}; expected contiguous [{H}, {D}] and [4] on {x.device}")
    lib = _lib.load()
    sizer = lib.qsaew_encode_topk_prefilter_workspace_bytes if pref else lib.qsaew_encode_topk_workspace_bytes
    need = int(sizer(max(B, 1), D, H, k, slab))
    if need == 0:
        raise ValueError(f"{who}: shape B={B}, D={D}, H={H}, k={k}, slab={slab} is outside what the slab selection runs (D % 4 == 0, "
                         f"H % 4 == 0, H <= 2^20, k <= 256, at most {WIDE_MAX_SLABS} slabs of at least k units)")
    idx = torch.empty((B, k), dtype=torch.int32, device=x.device)
    val = torch.empty((B, k), dtype=torch.float32, device=x.device)
    dense = torch.empty((B, H), dtype=torch.float32, device=x.device) if want_dense else None
    flagged = C.c_int(0)
    if B > 0:
        ws = _workspace(x.device, need)
        if pref:
            check(lib.qsaew_encode_topk_prefilter(_p(x), _p(W), _p(b), _p(Wq), _p(meta), B, D, H, k, slab, _p(idx), _p(val), _p(dense), H,
                                                  _p(ws), ws.numel(), int(spec_rows), C.byref(flagged), _stream()))
        else:
            check(lib.qsaew_encode_topk(_p(x), _p(W), _p(b), B, D, H, k, slab, _p(idx), _p(val), _p(dense), H, _p(ws), ws.numel(),
                                        _stream()))
    if info is not None:
        info["flagged_rows"] = int(flagged.value)
        info["slabs"] = len(starts) - 1
    return idx, val, dense
