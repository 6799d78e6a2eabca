"""What the Python wrappers of the multi-level objectives (nested levels, Multi-TopK points, ragged BatchTopK rows, nested levels
over ragged rows) refuse, and in which words: every case is one bad argument at the smallest shape that reaches the check
(B = 2, K = 4, H = 8, D = 4, n_bits = 4, bounds [4, 8], ks [2, 4]), raises before any launch, and is held against the
complete message, not a fragment of it.  The wrappers share their checks (ops._decode_sparse, _row_grad_levels,
_unit_grad_levels, _table_unit_grad_levels); the words, the exception types and the irregular cases -- a prefix here and none
there, a rank check one family has and the other leaves to the unpacking -- are part of what callers see."""
import pytest
import torch

from quantizedsae_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, K, H, D, N_BITS = 2, 4, 8, 4, 4
BOUNDS, KS = [4, 8], [2, 4]
I32, I64, F32, F64, U8 = torch.int32, torch.int64, torch.float32, torch.float64, torch.uint8
TRAIN_SHAPE = "BinarySAE training kernels take D a multiple of 4 up to 4096 and k <= 256 (got D = {}, k = {})"
UNPACK = "not enough values to unpack (expected 2, got 1)"


class z:
    """a zero tensor of this shape, made on the device when the case runs; strided: every second element of a last dimension
    twice as long"""

    def __init__(self, *shape, dtype=F32, strided=False):
        self.shape, self.dtype, self.strided = shape, dtype, strided

    def make(self):
        if not self.strided:
            return torch.zeros(self.shape, dtype=self.dtype, device=DEV)
        return torch.zeros(self.shape[:-1] + (2 * self.shape[-1],), dtype=self.dtype, device=DEV)[..., ::2]


def made(v):
    return v.make() if isinstance(v, z) else [made(e) for e in v] if isinstance(v, list) else v


def good(**changes):
    """the operands of a call that would pass, with ``changes`` applied"""
    o = dict(idx=z(B, K, dtype=I32), val=z(B, K), counts=z(B, dtype=I32), packed=z(H, 4, dtype=U8), table=z(H, D), D=D,
             n_bits=N_BITS, bias=z(D), bounds=BOUNDS, ks=KS, g=[z(B, D), z(B, D)], g_recon=z(B, D), g_latent=None,
             W_enc=z(H, D), want_dx=True, offsets=z(H + 1, dtype=I32), entries=z(B * K, dtype=I32), gv=z(B, K), x=z(B, D),
             G=z(2, B, D), logits=z(H, D * N_BITS))
    o.update(changes)
    return {name: made(v) for name, v in o.items()}


# how each public wrapper takes the operands of good(); "lv" is bounds or ks
def _decode_binary(fn, ragged, lv):
    def call(o):
        lists = (o["idx"], o["val"]) + ((o["counts"],) if ragged else ())
        return fn(*lists, o["packed"], o["D"], o["n_bits"], 0.5, o["bias"], *((o[lv],) if lv else ()))
    return call


def _decode_table(fn, ragged, lv):
    def call(o):
        lists = (o["idx"], o["val"]) + ((o["counts"],) if ragged else ())
        return fn(*lists, o["table"], 1.0, o["bias"], *((o[lv],) if lv else ()))
    return call


def _row_grad(fn, ragged, lv):
    def call(o):
        lists = (o["idx"],) + ((o["counts"],) if ragged else ())
        grads = (o["g"], o[lv]) if lv else (o["g_recon"],)
        return fn(*lists, o["table"], 1.0, *grads, o["g_latent"], o["W_enc"], o["want_dx"])
    return call


def _unit_grad(fn, lv):
    def call(o):
        return fn(o["offsets"], o["entries"], o["val"], o["gv"], o["x"], o["G"], o[lv], o["logits"], o["n_bits"], 0.5, None)
    return call


def _table_unit_grad(fn, lv):
    def call(o):
        return fn(o["offsets"], o["entries"], o["val"], o["gv"], o["x"], o["G"], o[lv])
    return call


CALLS = {
    "decode_nested_binary": _decode_binary(ops.decode_nested_binary, False, "bounds"),
    "decode_nested_table": _decode_table(ops.decode_nested_table, False, "bounds"),
    "decode_multik_binary": _decode_binary(ops.decode_multik_binary, False, "ks"),
    "decode_multik_table": _decode_table(ops.decode_multik_table, False, "ks"),
    "decode_ragged_binary": _decode_binary(ops.decode_ragged_binary, True, None),
    "decode_ragged_table": _decode_table(ops.decode_ragged_table, True, None),
    "decode_nested_ragged_binary": _decode_binary(ops.decode_nested_ragged_binary, True, "bounds"),
    "decode_nested_ragged_table": _decode_table(ops.decode_nested_ragged_table, True, "bounds"),
    "train_row_grad_nested": _row_grad(ops.train_row_grad_nested, False, "bounds"),
    "train_row_grad_multik": _row_grad(ops.train_row_grad_multik, False, "ks"),
    "train_row_grad_ragged": _row_grad(ops.train_row_grad_ragged, True, None),
    "train_row_grad_nested_ragged": _row_grad(ops.train_row_grad_nested_ragged, True, "bounds"),
    "train_unit_grad_nested": _unit_grad(ops.train_unit_grad_nested, "bounds"),
    "train_unit_grad_multik": _unit_grad(ops.train_unit_grad_multik, "ks"),
    "train_table_unit_grad_nested": _table_unit_grad(ops.train_table_unit_grad_nested, "bounds"),
    "train_table_unit_grad_multik": _table_unit_grad(ops.train_table_unit_grad_multik, "ks"),
}

NESTED_END = " must be ascending and distinct, start above 0 and end at hidden_dim = 8"
MULTIK_END = " must be ascending and distinct, start above 0 and end at the list width K = 4"


def level_cases(who, key):
    """the refusals of the host array: bounds (ending at H = 8) or ks (ending at K = 4)"""
    if key == "bounds":
        name, noun, end, not_asc, not_end, frac = "bounds", "levels", NESTED_END, [8, 8], [4, 6], [4.5, 8]
    else:
        name, noun, end, not_asc, not_end, frac = "ks", "points", MULTIK_END, [4, 4], [2, 3], [2.5, 4]
    return [
        (who, {key: not_asc}, ValueError, f"{who}: {name} = {not_asc}{end}"),
        (who, {key: not_end}, ValueError, f"{who}: {name} = {not_end}{end}"),
        (who, {key: [0, not_asc[0]]}, ValueError, f"{who}: {name} = {[0, not_asc[0]]}{end}"),
        (who, {key: frac}, ValueError, f"{who}: {name} must be whole numbers, got {frac}"),
        (who, {key: [True, not_asc[0]]}, ValueError, f"{who}: {name} must be whole numbers, got {[True, not_asc[0]]}"),
        (who, {key: 5}, ValueError, f"{who}: {name} must be a sequence of ints, got 5"),
        (who, {key: []}, ValueError, f"{who}: 0 {noun}; 1 .. 8 are supported"),
        (who, {key: list(range(1, 10))}, ValueError, f"{who}: 9 {noun}; 1 .. 8 are supported"),
    ]


def dictionary_cases(who, packed):
    """the refusals of the dictionary operand and the bias of a decoder"""
    d_text = "{}: D = {} must be a positive multiple of 4 up to 4096"
    out = [(who, {"bias": z(5)}, ValueError, f"{who}: bias is (5,), expected [4]")]
    if packed:
        out += [
            (who, {"packed": z(H, 4)}, TypeError, f"{who}: packed: expected dtype torch.uint8, got torch.float32"),
            (who, {"D": 6}, ValueError, d_text.format(who, 6)),
            (who, {"D": 4100}, ValueError, d_text.format(who, 4100)),
            (who, {"D": 0}, ValueError, d_text.format(who, 0)),
            (who, {"n_bits": 0}, ValueError, f"{who}: n_bits = 0 is outside 1 .. 8"),
            (who, {"n_bits": 9}, ValueError, f"{who}: n_bits = 9 is outside 1 .. 8"),
            (who, {"packed": z(H, 5, dtype=U8)}, ValueError, f"{who}: packed is (8, 5), expected contiguous [H, 4] on {DEV}"),
            (who, {"packed": z(H * 4, dtype=U8)}, ValueError, f"{who}: packed is (32,), expected contiguous [H, 4] on {DEV}"),
            (who, {"packed": z(H, 4, dtype=U8, strided=True)}, ValueError,
             f"{who}: packed is (8, 4), expected contiguous [H, 4] on {DEV}"),
        ]
    else:
        out += [
            (who, {"table": z(H * D)}, ValueError, f"{who}: table is (32,) on {DEV}, expected [H, D] on {DEV}"),
            (who, {"table": z(H, 6)}, ValueError, d_text.format(who, 6)),
            (who, {"table": z(H, 4100)}, ValueError, d_text.format(who, 4100)),
        ]
    return out


def build_cases():
    cases = []
    for fam, key in (("nested", "bounds"), ("multik", "ks")):
        for form in ("binary", "table"):
            who = f"decode_{fam}_{form}"
            lists = "{}: idx is {}, val {}; expected two [B, k] tensors on one device"
            cases += [
                (who, {"idx": z(B, K, dtype=I64)}, TypeError, f"{who}: idx: expected dtype torch.int32, got torch.int64"),
                (who, {"val": z(B, K, dtype=F64)}, TypeError, f"{who}: val: expected dtype torch.float32, got torch.float64"),
                (who, {"idx": z(B * K, dtype=I32), "val": z(B * K)}, ValueError, lists.format(who, "(8,)", "(8,)")),
                (who, {"val": z(B, 3)}, ValueError, lists.format(who, "(2, 4)", "(2, 3)")),
                (who, {"idx": z(B, 257, dtype=I32), "val": z(B, 257)}, ValueError, f"{who}: k = 257 exceeds 256"),
            ] + dictionary_cases(who, form == "binary") + level_cases(who, key)
        cases.append((f"decode_multik_{form}", {"idx": z(B, 0, dtype=I32), "val": z(B, 0), "ks": []}, ValueError,
                      f"decode_multik_{form}: 0 points; 1 .. 8 are supported"))
    for fam, key in (("ragged", None), ("nested_ragged", "bounds")):
        for form in ("binary", "table"):
            who = f"decode_{fam}_{form}"
            cases += [
                (who, {"idx": z(B, K, dtype=I64)}, TypeError, f"{who}: idx: expected dtype torch.int32, got torch.int64"),
                (who, {"counts": z(B, dtype=I64)}, TypeError, f"{who}: counts: expected dtype torch.int32, got torch.int64"),
                (who, {"val": z(B, K, dtype=F64)}, TypeError, f"{who}: val: expected dtype torch.float32, got torch.float64"),
                (who, {"val": z(B * K)}, ValueError, f"{who}: val is (8,), expected [B, K] with K >= 1"),
                (who, {"val": z(B, 0)}, ValueError, f"{who}: val is (2, 0), expected [B, K] with K >= 1"),
                (who, {"idx": z(B, 257, dtype=I32), "val": z(B, 257)}, ValueError, f"{who}: the cap K = 257 exceeds 256"),
                (who, {"val": z(B, 3)}, ValueError,
                 f"{who}: idx is (2, 4), val (2, 3); expected two [B, K] tensors on one device"),
                (who, {"counts": z(3, dtype=I32)}, ValueError, f"{who}: counts is (3,) on {DEV}, expected [2] on {DEV}"),
            ] + dictionary_cases(who, form == "binary") + (level_cases(who, key) if key else [])

    for who, key, grads, noun in (("train_row_grad_nested", "bounds", "g_levels", "level"),
                                  ("train_row_grad_multik", "ks", "g_points", "point"),
                                  ("train_row_grad_nested_ragged", "bounds", "g_levels", "level")):
        ragged = who.endswith("ragged")
        wide = (f"{who}: idx is (2, 257), expected [B, K] with 1 <= K <= 256" if ragged else TRAIN_SHAPE.format(4, 257))
        flat = {"train_row_grad_nested": UNPACK, "train_row_grad_multik": f"{who}: idx is (8,), expected [B, K]",
                "train_row_grad_nested_ragged": f"{who}: idx is (8,), expected [B, K] with 1 <= K <= 256"}[who]
        d_bad = (f"{who}: D = 6 must be a positive multiple of 4 up to 4096" if ragged else TRAIN_SHAPE.format(6, 4))
        d_wide = (f"{who}: D = 4100 must be a positive multiple of 4 up to 4096" if ragged else TRAIN_SHAPE.format(4100, 4))
        cases += [
            (who, {"idx": z(B, K, dtype=I64)}, TypeError, f"{who}: idx: expected dtype torch.int32, got torch.int64"),
            (who, {"idx": z(B * K, dtype=I32)}, ValueError, flat),
            (who, {"idx": z(B, 257, dtype=I32)}, ValueError, wide),
            (who, {"table": z(H, 6)}, ValueError, d_bad),
            (who, {"table": z(H, 4100)}, ValueError, d_wide),
            (who, {"g": [z(B, D)]}, ValueError, f"{who}: 1 {noun} gradients for 2 {noun}s"),
            (who, {"g": [z(B, D)] * 3}, ValueError, f"{who}: 3 {noun} gradients for 2 {noun}s"),
            (who, {"g": [None, z(B, 5)]}, ValueError, f"{who}: {grads}[1] is (2, 5) on {DEV}, expected [2, 4] on {DEV}"),
            (who, {"g": [z(B * D), None]}, ValueError, f"{who}: {grads}[0] is (8,) on {DEV}, expected [2, 4] on {DEV}"),
            (who, {"g_latent": z(B, 7)}, ValueError, "g_latent is (2, 7), expected [2, 8]"),
            (who, {"W_enc": z(H, 5)}, ValueError, "W_enc is (8, 5), expected [8, 4]"),
            (who, {"W_enc": z(D, H)}, ValueError, "W_enc is (4, 8), expected [8, 4]"),
        ] + level_cases(who, key)
        if ragged:
            cases += [
                (who, {"counts": z(B, dtype=I64)}, TypeError, f"{who}: counts: expected dtype torch.int32, got torch.int64"),
                (who, {"counts": z(3, dtype=I32)}, ValueError, f"{who}: counts is (3,) on {DEV}, expected [2] on {DEV}"),
            ]
    who = "train_row_grad_ragged"
    cases += [
        (who, {"idx": z(B, K, dtype=I64)}, TypeError, f"{who}: idx: expected dtype torch.int32, got torch.int64"),
        (who, {"counts": z(B, dtype=I64)}, TypeError, f"{who}: counts: expected dtype torch.int32, got torch.int64"),
        (who, {"idx": z(B * K, dtype=I32)}, ValueError, f"{who}: idx is (8,), expected [B, K] with 1 <= K <= 256"),
        (who, {"idx": z(B, 257, dtype=I32)}, ValueError, f"{who}: idx is (2, 257), expected [B, K] with 1 <= K <= 256"),
        (who, {"counts": z(3, dtype=I32)}, ValueError, f"{who}: counts is (3,) on {DEV}, expected [2] on {DEV}"),
        (who, {"table": z(H, 6)}, ValueError, f"{who}: D = 6 must be a positive multiple of 4 up to 4096"),
        (who, {"table": z(H, 4100)}, ValueError, f"{who}: D = 4100 must be a positive multiple of 4 up to 4096"),
        (who, {"g_recon": z(B, 5)}, ValueError, "g_recon is (2, 5), expected [2, 4]"),
        (who, {"g_latent": z(B, 7)}, ValueError, "g_latent is (2, 7), expected [2, 8]"),
        (who, {"W_enc": z(H, 5)}, ValueError, "W_enc is (8, 5), expected [8, 4]"),
    ]

    for fam, key, k_name in (("nested", "bounds", "k"), ("multik", "ks", "K")):
        for table in (False, True):
            who = f"train_{'table_' if table else ''}unit_grad_{fam}"
            ranks = f"{who}: val and x must be 2-D, offsets 1-D"
            early = table or fam == "multik"              # the packed nested form leaves the ranks to the unpacking
            cases += [
                (who, {"offsets": z(H + 1, dtype=I64)}, TypeError, "offsets: expected dtype torch.int32, got torch.int64"),
                (who, {"entries": z(B * K, dtype=I64)}, TypeError, "entries: expected dtype torch.int32, got torch.int64"),
                (who, {"val": z(B * K)}, ValueError, ranks if early else UNPACK),
                (who, {"val": z(B, 257), "gv": z(B, 257)}, ValueError, TRAIN_SHAPE.format(4, 257)),
                (who, {"x": z(B, 6)}, ValueError, TRAIN_SHAPE.format(6, 4)),
                (who, {"x": z(B, 4100)}, ValueError, TRAIN_SHAPE.format(4100, 4)),
                (who, {"gv": z(B, 3)}, ValueError, f"{who}: inconsistent shapes"),
                (who, {"x": z(3, D)}, ValueError, f"{who}: inconsistent shapes"),
                (who, {"entries": z(B * K + 1, dtype=I32)}, ValueError, f"{who}: inconsistent shapes"),
                (who, {"G": z(2, B, D, dtype=F64)}, TypeError, f"{who}: G: expected dtype torch.float32, got torch.float64"),
                (who, {"G": z(3, B, D)}, ValueError, f"{who}: G is (3, 2, 4) (strides (8, 4, 1)), expected contiguous [2, 2, 4]"),
                (who, {"G": z(2, B, D, strided=True)}, ValueError,
                 f"{who}: G is (2, 2, 4) (strides (16, 8, 2)), expected contiguous [2, 2, 4]"),
            ] + level_cases(who, key)
            if early:
                cases.append((who, {"offsets": z(1, dtype=I32), "logits": z(0, D * N_BITS)}, ValueError,
                              f"{who}: inconsistent shapes"))
            if not table:
                cases.append((who, {"logits": z(H, D * N_BITS + 1)}, ValueError, f"{who}: inconsistent shapes"))
    return cases


def case_ids():
    return [f"{who}-{'+'.join(changes)}-{i}" for i, (who, changes, _, _) in enumerate(build_cases())]


def test_every_public_wrapper_has_cases():
    assert {c[0] for c in build_cases()} == set(CALLS)


@pytest.mark.parametrize("who, changes, exc, text", build_cases(), ids=case_ids())
def test_refusal_word_for_word(who, changes, exc, text):
    with pytest.raises(exc) as e:
        CALLS[who](good(**changes))
    assert type(e.value) is exc and str(e.value) == text


@pytest.mark.parametrize("call, text", [
    (lambda: ops.nested_bounds([4, 6], 8), "nested_bounds: bounds = [4, 6]" + NESTED_END),
    (lambda: ops.nested_bounds([8, 4], 8), "nested_bounds: bounds = [8, 4]" + NESTED_END),
    (lambda: ops.nested_bounds([4.5, 8], 8), "nested_bounds: bounds must be whole numbers, got [4.5, 8]"),
    (lambda: ops.nested_bounds(5, 8), "nested_bounds: bounds must be a sequence of ints, got 5"),
    (lambda: ops.nested_bounds([], 8), "nested_bounds: 0 levels; 1 .. 8 are supported"),
    (lambda: ops.nested_bounds(range(1, 10), 9), "nested_bounds: 9 levels; 1 .. 8 are supported"),
    (lambda: ops.nested_bounds([4, 8], 8, "Model.forward_nested"), None),
    (lambda: ops.multik_points([2, 3], 4), "multik_points: ks = [2, 3]" + MULTIK_END),
    (lambda: ops.multik_points([4, 4], 4), "multik_points: ks = [4, 4]" + MULTIK_END),
    (lambda: ops.multik_points([2.5, 4], 4), "multik_points: ks must be whole numbers, got [2.5, 4]"),
    (lambda: ops.multik_points(None, 4), "multik_points: ks must be a sequence of ints, got None"),
    (lambda: ops.multik_points([], 4), "multik_points: 0 points; 1 .. 8 are supported"),
    (lambda: ops.multik_points(range(1, 10), 9), "multik_points: 9 points; 1 .. 8 are supported"),
    (lambda: ops.multik_points([2, 300], 300), "multik_points: the list width K = 300 is outside 1 .. 256"),
    (lambda: ops.multik_points([2], 0, "who"), "who: the list width K = 0 is outside 1 .. 256"),
    (lambda: ops.multik_points([2, 4], 4, "Model.forward_multi_topk"), None),
])
def test_level_validators_word_for_word(call, text):
    if text is None:
        assert call() == [2, 4] or call() == [4, 8]
        return
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == text
