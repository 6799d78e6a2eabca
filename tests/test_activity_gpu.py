"""Per-feature firing counts on the GPU (csrc/activity.hip, quantizedsae_amd.training.activity): the four kernels bit for bit
against the numpy restatement of tests/activity_util.py and against torch's ``(latent > 0).sum(0)``, every entry point
between guard words, the hooks of the six model classes against the reference's activation mask, and the Trainer's
``activity_window``.  Everything is integer: every comparison is exact."""
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import activity_util as U  # noqa: E402
import guard_util as GU  # noqa: E402
import trainer_util as TU  # noqa: E402
from guard_util import STREAM, WS, WS_BYTES, Buf, Call, HostArray  # noqa: E402
from quantizedsae_amd import _lib, ops  # noqa: E402
from quantizedsae_amd import torch_ops  # noqa: E402,F401
from quantizedsae_amd.inference import analysis  # noqa: E402
from quantizedsae_amd.training import FeatureActivity, Trainer, trainer_loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I64, I32, F32 = torch.int64, torch.int32, torch.float32


@pytest.fixture(autouse=True)
def _grad_mode_on():
    with torch.enable_grad():
        yield


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t) -> np.ndarray:
    return t.detach().cpu().numpy()


def zeros(H):
    return np.zeros(H, np.int64)


def check_add(kind, want, args, H, stamp=5, fired0=None, last0=None):
    """One add on the device from the given start state -> compared with the restatement's (fired, last)"""
    fired0 = zeros(H) if fired0 is None else fired0
    last0 = zeros(H) if last0 is None else last0
    fired, last = dev(fired0), dev(last0)
    getattr(ops, f"activity_add_{kind}")(*args, stamp, fired, last)
    wf, wl = want(fired0, last0, stamp)
    assert np.array_equal(host(fired), wf), kind
    assert np.array_equal(host(last), wl), kind
    return host(fired), host(last)


# ---- compact ---------------------------------------------------------------------------------------------------------------------
def test_compact_minimal():
    for v, on in ((1.0, 1), (-1.0, 0), (0.0, 0), (np.nan, 0)):
        idx, val = np.zeros((1, 1), np.int32), np.full((1, 1), v, np.float32)
        f, l = check_add("compact", lambda f, l, s: U.add_compact(idx, val, 1, s, f, l), (dev(idx), dev(val)), 1)
        assert f.tolist() == [on] and l.tolist() == [5 * on]
    idx = np.zeros((1, 1), np.int32)
    f, _ = check_add("compact", lambda f, l, s: U.add_compact(idx, None, 1, s, f, l), (dev(idx), None), 1)
    assert f.tolist() == [1]


def test_compact_tails_with_dropped_indices_special_values_and_repeats():
    B, k, H = 257, 65, 1000
    idx, val = U.compact_case(B, k, H)
    assert (idx == -1).any() and (idx == H).any() and np.isnan(val).any() and (val < 0).any()
    assert np.signbit(val[2, 2]) and val[2, 2] == 0 and val[2, 1] == 0 and (idx[4] == 5).all()
    f, l = check_add("compact", lambda f, l, s: U.add_compact(idx, val, H, s, f, l), (dev(idx), dev(val)), H)
    # the torch one-liner on the dense mask (no unit repeats inside a row apart from the planted ones, which count twice)
    mask = torch.zeros((B, H + 1), dtype=I64)
    ok = torch.from_numpy((idx >= 0) & (idx < H)) & (torch.from_numpy(val) > 0)
    mask.index_put_((torch.arange(B)[:, None].expand(B, k)[ok], torch.from_numpy(idx).long()[ok]), torch.ones((), dtype=I64),
                    accumulate=True)
    assert np.array_equal(f, mask[:, :H].sum(0).numpy())
    assert f[5] >= k and f[7] >= 2                          # a unit listed k times in a row counts k times
    assert np.array_equal(l, np.where(f > 0, 5, 0))
    # val = None: every listed entry
    f2, _ = check_add("compact", lambda f, l, s: U.add_compact(idx, None, H, s, f, l), (dev(idx), None), H)
    assert f2.sum() == B * k - 3                            # all but the three indices outside [0, H)


# ---- bits --------------------------------------------------------------------------------------------------------------------------
def test_bits_minimal_and_identity():
    z = np.array([[0x80000005 - (1 << 32)]], np.int32)
    f, l = check_add("bits", lambda f, l, s: U.add_bits(z, 32, None, 32, s, f, l), (dev(z), None), 32)
    assert np.flatnonzero(f).tolist() == [0, 2, 31] and np.flatnonzero(l).tolist() == [0, 2, 31]
    # index = None with H == nbits, more than one word column block and more rows than one pass of the row groups
    B, words = 1100, 70
    z = U.bits_case(B, words, words, density=0.1)
    H = 32 * words
    f, _ = check_add("bits", lambda f, l, s: U.add_bits(z, H, None, H, s, f, l), (dev(z), None), H)
    assert np.array_equal(f, U.bits_mask(z, H).sum(0))
    assert np.array_equal(f, host(ops.activation_counts_bits(dev(z))))


def test_bits_tails_with_a_row_stride_and_a_padded_permutation():
    B, words, ld, H = 130, 5, 7, 140
    z = U.bits_case(B, words, ld)
    index = U.padded_index(32 * words, H)
    pads = np.flatnonzero(index < 0)
    assert pads.size == 20 and U.bits_mask(z, 160)[:, pads].any()           # the pad slots' bits are set
    zd = dev(z)[:, :words]
    assert zd.stride(0) == ld
    f, l = check_add("bits", lambda f, l, s: U.add_bits(z, 160, index, H, s, f, l), (zd, dev(index)), H)
    dense = np.zeros((B, H), bool)
    dense[:, index[index >= 0]] = U.bits_mask(z, 160)[:, index >= 0]
    assert np.array_equal(f, torch.from_numpy(dense).sum(0).numpy())
    # an int64 map, and values >= H dropped
    index2 = index.copy()
    index2[index2 == 3] = H
    f2, _ = check_add("bits", lambda f, l, s: U.add_bits(z, 160, index2, H, s, f, l), (zd, dev(index2.astype(np.int64))), H)
    assert f2[3] == 0 and np.array_equal(np.delete(f2, 3), np.delete(f, 3))


# ---- dense -------------------------------------------------------------------------------------------------------------------------
def test_dense_minimal():
    for v, on in ((1.0, 1), (0.0, 0), (-0.0, 0), (np.nan, 0), (np.inf, 1), (1e-45, 1), (-np.inf, 0)):
        x = np.full((1, 1), v, np.float32)
        f, l = check_add("dense", lambda f, l, s: U.add_dense(x, 1, s, f, l), (dev(x),), 1)
        assert f.tolist() == [on] and l.tolist() == [5 * on], v


@pytest.mark.parametrize("shape", [(67, 1029, 1040), (67, 1029, 1029), (1030, 300, 300)], ids=lambda s: "x".join(map(str, s)))
def test_dense_tails_with_special_values(shape):
    """ld = 1040: 16-byte loads with a scalar tail quad; ld = 1029: rows off their 16-byte boundary, scalar loads; 1030 rows:
    more than one workgroup of 256 rows"""
    B, H, ld = shape
    x = U.dense_case(B, H, ld)
    assert np.isnan(x[1, 0]) and np.signbit(x[1, 1]) and np.isinf(x[1, 2]) and 0 < x[1, 4] < 1e-38
    xd = dev(x)[:, :H]
    f, l = check_add("dense", lambda f, l, s: U.add_dense(x, H, s, f, l), (xd,), H)
    assert np.array_equal(f, host((xd > 0).sum(0)))
    assert f[5] == 0 and l[5] == 0 and f[H - 1] == B and f[0] == (x[:, 0] > 0).sum()
    # a view that starts off its 16-byte boundary gives the same counts
    flat = torch.zeros(B * ld + 1, device=DEV)
    flat[1:] = dev(x).reshape(-1)
    off = flat[1:].view(B, ld)[:, :H]
    assert off.data_ptr() % 16 == 4
    f2, _ = check_add("dense", lambda f, l, s: U.add_dense(x, H, s, f, l), (off,), H)
    assert np.array_equal(f2, f)


def test_a_unit_that_does_not_fire_is_not_written():
    H = 64
    x = np.zeros((3, H), np.float32)
    x[:, 1] = 1.0
    fired0, last0 = np.full(H, 7, np.int64), np.full(H, 99, np.int64)
    f, l = check_add("dense", lambda f, l, s: U.add_dense(x, H, s, f, l), (dev(x),), H, stamp=5, fired0=fired0, last0=last0)
    assert f[1] == 10 and (np.delete(f, 1) == 7).all() and (l == 99).all()   # a smaller stamp does not lower last


# ---- state ---------------------------------------------------------------------------------------------------------------------------
def _sequence():
    H = 1000
    batches = [U.compact_case(64, 9, H, seed=s, specials=False) for s in (11, 12, 13, 14)]
    stamps = [64, 128, 192, 100]                             # the fourth arrives out of order
    fired0 = zeros(H)
    fired0[3] = 2 ** 32 - 1                                  # the next add carries into the high word
    batches[0][0][0, 0], batches[0][1][0, 0] = 3, 1.0
    return H, batches, stamps, fired0


def _run_sequence():
    H, batches, stamps, fired0 = _sequence()
    fired, last = dev(fired0), dev(zeros(H))
    trail = []
    for (idx, val), s in zip(batches, stamps):
        ops.activity_add_compact(dev(idx), dev(val), s, fired, last)
        trail.append((host(fired), host(last)))
    return trail


def test_stamps_never_go_down_counts_carry_and_a_second_run_gives_the_same_bits():
    H, batches, stamps, fired0 = _sequence()
    trail = _run_sequence()
    wf, wl = fired0, zeros(H)
    for (idx, val), s, (gf, gl) in zip(batches, stamps, trail):
        before = wl
        wf, wl = U.add_compact(idx, val, H, s, wf, wl)
        assert np.array_equal(gf, wf) and np.array_equal(gl, wl) and (gl >= before).all()
    assert trail[-1][0][3] >= 2 ** 32 and trail[-1][1].max() == 192 and (trail[-1][1] == 100).any()
    again = _run_sequence()
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(trail, again))


def test_the_adds_do_not_wait_for_the_device():
    H = 96
    t = FeatureActivity(H, DEV)
    idx, val = (dev(a) for a in U.compact_case(48, 5, H, specials=False))
    z, x = dev(U.bits_case(48, 3, 3)), dev(U.dense_case(48, H, H, specials=False))
    for _ in range(2):                                       # the first round loads the kernels
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            t.add_compact(idx, val)
            t.add_bits(z)
            t.add_dense(x)
            t.segment(32, 64).add_bits(z[:, :2])
        finally:
            torch.cuda.set_sync_debug_mode("default")
    # the segment does not advance the clock: its batch is stamped as the next one of the owner would be
    assert t.rows_seen == 6 * 48 and int(t.last[:32].max()) == 6 * 48 and int(t.last[32:].max()) == 7 * 48


# ---- summary -------------------------------------------------------------------------------------------------------------------------
SEGMENTS = {0: [], 1: [2500], 4: [37, 1203, 1, 1259]}


@pytest.mark.parametrize("advance", [0, 1])
@pytest.mark.parametrize("n_seg", sorted(SEGMENTS))
def test_summary_equals_the_restatement(n_seg, advance):
    H, clock, window = 2500, 5000, 700
    fired, base, last = U.state_case(H)
    fired[17] = 2 ** 32 + 5                                  # an interval count in the last octave
    base[17] = 0
    sizes = SEGMENTS[n_seg]
    want, want_dead = U.summary(fired, base, last, clock, window, sizes)
    assert 0 < want_dead.size < H and want[0, U.HEAD + 33] == 1 and (want[0, U.HEAD:] > 0).sum() > 12
    df, db, dl = dev(fired), dev(base), dev(last)
    dead_out = torch.full((H,), U.DEAD_POISON, dtype=I32, device=DEV)
    res = ops.activity_summary(df, db, dl, clock, window, sizes, bool(advance), dead_out)
    assert res.dtype == I64 and tuple(res.shape) == (1 + n_seg, U.WORDS)
    assert np.array_equal(host(res), want)
    assert np.array_equal(host(df), fired) and np.array_equal(host(dl), last)
    assert np.array_equal(host(db), fired if advance else base)
    n = int(res[0, U.DEAD])
    got = host(dead_out)
    assert n == want_dead.size and np.array_equal(got[:n], want_dead) and (np.diff(got[:n]) > 0).all()
    assert (got[n:] == U.DEAD_POISON).all()                  # the tail is left untouched
    # the same through the dispatcher, without a list; a second call gives the same bits
    res2 = torch_ops.activity_summary(df, db, dl, clock, window, sizes, False, None)
    assert np.array_equal(host(res2), U.summary(fired, fired if advance else base, last, clock, window, sizes)[0])


def test_summary_without_a_base_and_at_one_unit():
    fired, _, last = U.state_case(1500, seed=9)
    want, want_dead = U.summary(fired, None, last, 5000, 1, [])
    dead_out = torch.full((1500,), U.DEAD_POISON, dtype=I32, device=DEV)
    res = ops.activity_summary(dev(fired), None, dev(last), 5000, 1, (), True, dead_out)
    assert np.array_equal(host(res), want) and np.array_equal(host(dead_out)[:want_dead.size], want_dead)
    assert want[0, U.SUM_INTERVAL] == want[0, U.SUM_FIRED] == fired.sum()
    for clock, dead in ((9, 0), (10, 1)):                    # a never-fired unit before and after clock >= W
        res = ops.activity_summary(dev(zeros(1)), None, dev(zeros(1)), clock, 10)
        assert host(res)[0, :4].tolist() == [1, 1, dead, 1]


def test_an_undersized_workspace_is_refused_with_nothing_written():
    H = 70000
    lib = _lib.load()
    need = int(lib.qsae_activity_summary_workspace_bytes(H))
    assert need == U.workspace_bytes(H) == 512
    fired, base, last = (dev(a) for a in U.state_case(H))
    result = torch.full((U.WORDS,), 77, dtype=I64, device=DEV)
    dead_out = torch.full((H,), U.DEAD_POISON, dtype=I32, device=DEV)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    before = host(base).copy()
    p = lambda t: t.data_ptr()  # noqa: E731
    rc = lib.qsae_activity_summary(p(fired), p(base), p(last), H, 5000, 700, None, 0, 1, p(result), p(dead_out), p(ws), need - 1, None)
    torch.cuda.synchronize()
    assert rc == _lib.ERR_WORKSPACE
    assert (host(result) == 77).all() and (host(dead_out) == U.DEAD_POISON).all() and np.array_equal(host(base), before)
    rc = lib.qsae_activity_summary(p(fired), p(base), p(last), H, 5000, 700, None, 0, 1, p(result), p(dead_out), p(ws), need, None)
    torch.cuda.synchronize()
    assert rc == _lib.OK and int(result[0]) == H


# ---- guards --------------------------------------------------------------------------------------------------------------------------
def _state_bufs(H, seed):
    fired, _, last = U.state_case(H, seed=seed)
    return Buf("fired", "inout", data=dev(fired)), Buf("last", "inout", data=dev(last))


def _front(restate):
    def front(t):
        f, l = restate({k: host(v) for k, v in t.items()})
        return {"fired": dev(f), "last": dev(l)}
    return front


ENTRY_POINTS = {"qsae_activity_add_compact", "qsae_activity_add_bits", "qsae_activity_add_dense", "qsae_activity_summary",
                "qsae_activity_summary_workspace_bytes"}


def guard_calls(shape):
    tails = shape == "tails"
    calls = []
    # compact
    B, k, H = (257, 65, 1000) if tails else (1, 1, 1)
    idx, val = U.compact_case(B, k, H, specials=tails)
    if not tails:
        idx[:], val[:] = 0, 1.0
    for with_val in (True, False):
        calls.append(Call(f"compact {B}x{k} H={H}" + ("" if with_val else " val=NULL"), "qsae_activity_add_compact",
                          [Buf("idx", "in", data=dev(idx)), Buf("val", "in", data=dev(val)) if with_val else None, B, k, H, 9,
                           *_state_bufs(H, 21), STREAM],
                          _front(lambda t, H=H, w=with_val: U.add_compact(t["idx"], t["val"] if w else None, H, 9, t["fired"], t["last"]))))
    # bits
    B, words, ld, H = (130, 5, 7, 140) if tails else (1, 1, 1, 32)
    z = U.bits_case(B, words, ld)
    index = U.padded_index(32 * words, H) if tails else None
    calls.append(Call(f"bits {B}x{words} ld={ld} H={H}", "qsae_activity_add_bits",
                      [Buf("zbits", "in", data=dev(z)), ld, B, 32 * words, Buf("index", "in", data=dev(index)) if tails else None,
                       H, 9, *_state_bufs(H, 22), STREAM],
                      _front(lambda t, H=H, n=32 * words, ix=index: U.add_bits(t["zbits"], n, ix, H, 9, t["fired"], t["last"]))))
    # dense
    B, H, ld = (67, 1029, 1040) if tails else (1, 1, 1)
    x = U.dense_case(B, H, ld, specials=tails)
    calls.append(Call(f"dense {B}x{H} ld={ld}", "qsae_activity_add_dense",
                      [Buf("latent", "in", data=dev(x)), ld, B, H, 9, *_state_bufs(H, 23), STREAM],
                      _front(lambda t, H=H: U.add_dense(t["latent"], H, 9, t["fired"], t["last"]))))
    # summary (its sizer is the fifth entry point)
    H, sizes = (2500, SEGMENTS[4]) if tails else (1, [])
    fired, base, last = U.state_case(H, seed=24)

    def summary_front(t, sizes=sizes, H=H):
        fired = host(t["fired"])
        res, dead = U.summary(fired, host(t["base"]), host(t["last"]), 5000, 700, sizes)
        out = np.full(H, U.DEAD_POISON, np.int32)
        out[:dead.size] = dead
        return {"base": dev(fired), "result": dev(res), "dead_out": dev(out)}
    calls.append(Call(f"summary H={H} n_seg={len(sizes)}", "qsae_activity_summary",
                      [Buf("fired", "in", data=dev(fired)), Buf("base", "inout", data=dev(base)), Buf("last", "in", data=dev(last)),
                       H, 5000, 700, HostArray(sizes) if sizes else None, len(sizes), 1,
                       Buf("result", "out", shape=(1 + len(sizes), U.WORDS), dtype=I64), Buf("dead_out", "out", shape=(H,), dtype=I32),
                       WS, WS_BYTES, STREAM],
                      summary_front, sizer=("qsae_activity_summary_workspace_bytes", (H,))))
    return calls


@pytest.mark.parametrize("shape", ["minimal", "tails"])
def test_entry_points_between_guards(shape):
    lib = _lib.load()
    calls = guard_calls(shape)
    assert {c.entry for c in calls} | {c.sizer[0] for c in calls if c.sizer} == ENTRY_POINTS
    for call in calls:
        GU.run_call(call, lib, DEV)
    assert int(lib.qsae_activity_summary_workspace_bytes(2500 if shape == "tails" else 1)) == 256


# ---- models --------------------------------------------------------------------------------------------------------------------------
MODEL_B, MODEL_D = 48, 64
MODEL_H = {"b_sae": 1000, "baseline_sae": 1000, "t_sae": 1000, "bl_sae": 992, "q_sae": 1000, "rq_sae": 1000}


def _model(sae_type, seed=31):
    from quantizedsae_amd.training.trainer import _build_model
    import train_matryoshka_util as M
    S, D, H = TU.S, MODEL_D, MODEL_H[sae_type]
    cfg = dict(TU.epoch_config(), input_dim=D, hidden_dim=H)
    if sae_type == "b_sae":
        sd = S.binary_sae_params(seed, D, H, 8, dec_bias_std=0.05, logit_std=(2.0 / (D * 8)) ** 0.5)
    elif sae_type == "baseline_sae":
        sd = S.baseline_sae_params(seed, D, H)
    elif sae_type == "t_sae":
        sd = S.ternary_sae_params(seed, D, H)
    elif sae_type == "bl_sae":
        sd = TU._blatent_params(seed, D, H)
    elif sae_type == "q_sae":
        sd = M.q_params(seed, D, H, -1.0)
    else:
        sd = M.rq_params(seed, D, H, cfg["n_bits"], -1.0)
    model = _build_model(sae_type, cfg)
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys, res
    model = model.to(DEV)
    if sae_type == "t_sae":
        model.decoder.init_mask(TU.T_SPARSITY)
    return model, cfg


def _train_step(sae_type, model, cfg, x):
    """forward_train, the type's loss and backward -> (flat list of output tensors, grads by name)"""
    model.zero_grad(set_to_none=True)
    outputs = model.forward_train(x)
    trainer_loss(sae_type, outputs, x, cfg)
    flat = []
    for o in outputs:
        flat += list(o) if isinstance(o, (list, tuple)) else [o]
    return outputs, [t.detach().clone() for t in flat], {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _reference_mask(sae_type, model, outputs, x) -> torch.Tensor:
    """The reference's activation mask of the class, bool [B, H] on the device"""
    if sae_type in ("b_sae", "baseline_sae", "t_sae", "bl_sae"):
        return outputs[0].detach() > 0                       # ``latent > 0`` on the returned latent
    mask = analysis._activation_mask(types.SimpleNamespace(model=model, device=torch.device(DEV)), x)
    return mask.to(DEV)


@pytest.mark.parametrize("sae_type", TU.TYPES)
def test_forward_train_feeds_the_tracker_and_changes_nothing_else(sae_type):
    model, cfg = _model(sae_type)
    B, H = MODEL_B, MODEL_H[sae_type]
    x = dev(TU.S.activations(77, B, MODEL_D))
    assert model.activity is None
    _, outs0, grads0 = _train_step(sae_type, model, cfg, x)
    tracker = FeatureActivity.for_model(model)
    assert tracker.H == H and tracker.device == torch.device(DEV)
    model.activity = tracker
    outputs, outs1, grads1 = _train_step(sae_type, model, cfg, x)
    mask = _reference_mask(sae_type, model, outputs, x)
    assert tuple(mask.shape) == (B, H)
    want = mask.sum(0)
    assert 0 < int(want.sum()) < B * H
    assert torch.equal(tracker.fired, want)
    assert torch.equal(tracker.last, torch.where(want > 0, B, 0))
    assert tracker.rows_seen == B                            # also for rq_sae: the stages sit side by side, one batch
    if sae_type == "rq_sae":
        assert all("activity" not in s.__dict__ for s in model.saes)
        bounds = np.cumsum([0] + list(model.sae_hidden_dims))
        assert all(int(tracker.fired[a:b].sum()) > 0 for a, b in zip(bounds[:-1], bounds[1:]))
    # outputs and every gradient: the same bits as without the tracker
    assert len(outs0) == len(outs1) and all(GU.same_bits(a, b) for a, b in zip(outs0, outs1))
    assert sorted(grads0) == sorted(grads1) and len(grads0) >= 3 and all(GU.same_bits(grads0[n], grads1[n]) for n in grads0)
    # forward() leaves the tracker alone; a second forward_train adds the same counts again
    before = (tracker.fired.clone(), tracker.last.clone(), tracker.rows_seen)
    with torch.no_grad():
        model(x)
    assert torch.equal(tracker.fired, before[0]) and torch.equal(tracker.last, before[1]) and tracker.rows_seen == B
    model.forward_train(x)
    assert torch.equal(tracker.fired, 2 * want) and tracker.rows_seen == 2 * B
    assert torch.equal(tracker.last, torch.where(want > 0, 2 * B, 0))
    s = tracker.summary(B + 1, dead_list=True)
    assert s.units == H and s.never == int((want == 0).sum()) == s.dead == s.silent and s.interval_rows == 2 * B
    assert s.interval_count == 2 * int(want.sum()) and s.mean_l0 == s.interval_count / (2 * B)
    assert torch.equal(s.dead_indices.long(), torch.nonzero(want == 0).reshape(-1))
    assert [lv.units for lv in s.levels] == tracker.level_sizes and (not s.levels or sum(lv.dead for lv in s.levels) == s.dead)
    again = tracker.summary(B + 1)
    assert again.silent == H and again.interval_rows == 0 and again.mean_l0 == 0.0 and again.dead == s.dead
    # a resumed run keeps its clock and counts
    fresh = FeatureActivity.for_model(model)
    fresh.load_state_dict(tracker.state_dict())
    assert fresh.rows_seen == 2 * B and torch.equal(fresh.fired, tracker.fired) and torch.equal(fresh.base, tracker.base)


# ---- trainer -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def epoch_fixture():
    return TU.load_epoch_fixture()


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory, epoch_fixture):
    d = tmp_path_factory.mktemp("activity_dataset")
    torch.save(TU.epoch_chunk(epoch_fixture[0]["seed"]), d / TU.CHUNK_NAME)
    return d


def _epoch_model(sae_type, seed):
    from quantizedsae_amd.training.trainer import _build_model
    model = _build_model(sae_type, TU.epoch_config())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in TU.epoch_params(sae_type, seed).items()}, strict=False)
    return model.to(DEV)


def _run_epoch(sae_type, meta, dataset_dir, tmp_path, window, log_every, log_fn=True):
    logs, rows = [], []
    t = Trainer(TU.epoch_config(), sae_type, False, True, model=_epoch_model(sae_type, meta["seed"]), dataset_dir=str(dataset_dir),
                save_dir=str(tmp_path), log_fn=logs.append if log_fn else None, log_every=log_every, activity_window=window)
    step = t._step

    def spying_step(optimizer, batch, log_step):
        rows.append((int(batch.shape[0]), bool(log_step)))
        return step(optimizer, batch, log_step)
    t._step = spying_step
    torch.manual_seed(meta["seed"])
    t.one_epoch(str(dataset_dir / TU.CHUNK_NAME))
    return t, logs, rows


NEW_KEYS = {"dead_features", "dead_fraction", "never_fired", "silent_features", "mean_l0", "count_octaves"}


@pytest.mark.parametrize("sae_type", ["baseline_sae", "q_sae"])
def test_trainer_logs_the_activity_on_logging_steps_and_trains_the_same(sae_type, epoch_fixture, dataset_dir, tmp_path, capsys):
    meta, _ = epoch_fixture
    H, W = TU.EPOCH["H"], 100
    plain, logs0, rows0 = _run_epoch(sae_type, meta, dataset_dir, tmp_path, None, 2)
    t, logs, rows = _run_epoch(sae_type, meta, dataset_dir, tmp_path, W, 2)
    assert plain.activity is None and "activity" not in plain.model.__dict__ and t.model.activity is t.activity
    # the same batches, the same parameters bit for bit, the same reference metrics
    assert t.trained_batches == plain.trained_batches and rows == rows0 and len(rows) == 4
    sd0, sd1 = plain.model.state_dict(), t.model.state_dict()
    assert list(sd0) == list(sd1) and all(GU.same_bits(sd0[k], sd1[k]) for k in sd0)
    n_log = sum(1 for _, log_step in rows if log_step)
    assert len(logs) == len(logs0) == n_log and 0 < n_log < len(rows)            # logging steps only
    level_keys = {f"dead_features_level_{i}" for i in range(TU.EPOCH["n_bits"])} if sae_type == "q_sae" else set()
    for m0, m in zip(logs0, logs):
        assert set(m) == set(m0) | NEW_KEYS | level_keys and not (set(m0) & (NEW_KEYS | level_keys))
        assert all(m[k] == m0[k] for k in m0)
        assert len(m["count_octaves"]) == 34 and sum(m["count_octaves"]) == H and m["count_octaves"][0] == m["silent_features"]
        assert m["dead_fraction"] == m["dead_features"] / H and 0 <= m["dead_features"] <= m["silent_features"] + H
        if level_keys:
            assert sum(m[k] for k in level_keys) == m["dead_features"]
    # every interval's count is mean_l0 * its rows; with the rows after the last logging step they add up to fired.sum()
    total, pending, it = 0, 0, iter(logs)
    for n, log_step in rows:
        pending += n
        if log_step:
            total += round(next(it)["mean_l0"] * pending)
            pending = 0
    tail = t.activity.summary(W)
    assert tail.interval_rows == pending and t.activity.rows_seen == sum(n for n, _ in rows)
    assert total + tail.interval_count == int(t.activity.fired.sum()) > 0
    assert int(t.activity.last.max()) == t.activity.rows_seen
    # the tracker lives across one_epoch calls; under no_log the activity line follows the reference's line
    capsys.readouterr()
    epoch_rows = t.activity.rows_seen
    t.log_fn = None
    torch.manual_seed(meta["seed"])
    t.one_epoch(str(dataset_dir / TU.CHUNK_NAME))
    assert t.activity.rows_seen == 2 * epoch_rows
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(("Batch ", "  activity:")) and "NaN" not in ln]
    assert len(lines) == 2 * n_log
    for ref, act in zip(lines[0::2], lines[1::2]):
        assert ref.startswith("Batch ") and ("Loss=" in ref or "recon_loss_group_0=" in ref) and act.startswith("  activity: dead=")
