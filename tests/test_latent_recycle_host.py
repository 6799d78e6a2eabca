"""Recycled dense latents without a GPU: the ledger of include/qsae_recycle.h -- every function declared there is bound in
_lib.RECYCLE_SIGNATURES with as many arguments as it declares (its namesake's of qsae.h plus stale_idx, stale_k) and is
exported by the product and the debug library as qsaer_*; the calls of the C ABI that return before they look at a pointer;
and the pool of ops.py on CPU tensors: which holders of a latent keep it from being taken (a second name, a slice, a detached
alias, .numpy(), a DLPack capsule, a view kept in a list), which writes drop its record (an in-place op, a raw-pointer write
announced with _latent_pool_forget), the bound per device, release_workspaces(), and two threads on keys of their own."""
import re
import threading
from pathlib import Path

import pytest
import torch

from quantizedsae_amd import _lib, build, ops

ROOT = Path(__file__).resolve().parents[1]
NAMESAKES = ("qsae_binary_forward_prefilter", "qsae_table_forward_prefilter", "qsae_prefilter_submit", "qsae_prefilter_submit_table")


# ---- the ledger of the header -----------------------------------------------------------------------------------------
def _declared(header):
    """name -> parameter list of every function declared in include/<header>"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
    return {name: [p.strip() for p in params.split(",")] for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text)}


def test_every_declared_function_is_bound_and_exported():
    declared = _declared("qsae_recycle.h")
    assert len(declared) == 4 and sorted(declared) == sorted(_lib.RECYCLE_SIGNATURES)
    assert all(n.startswith("qsaer_") for n in declared)
    others = (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.CURVE_SIGNATURES, _lib.NESTED_SIGNATURES, _lib.BATCH_SIGNATURES,
              _lib.NESTED_BATCH_SIGNATURES, _lib.MULTIK_SIGNATURES, _lib.JUMP_SIGNATURES, _lib.JUMP_DENSE_SIGNATURES,
              _lib.BATCH_DENSE_SIGNATURES)
    assert not any(set(declared) & set(t) for t in others)
    assert not any(n.startswith("qsaer_") for t in others for n in t)
    base = _declared("qsae.h")
    for name, params in declared.items():
        namesake = "qsae_" + name[len("qsaer_"):]
        assert namesake in NAMESAKES
        assert params == base[namesake] + ["const int32_t* stale_idx", "int stale_k"], name      # the same arguments plus two
        res, args = _lib.RECYCLE_SIGNATURES[name]
        assert len(args) == len(params) and (res, args[:-2]) == tuple(_lib.SIGNATURES[namesake]), name
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert sorted(s for s in build.exported_symbols(path) if s.startswith("qsaer_")) == sorted(declared)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    assert _lib.ABI_VERSION == 4 and "join qsae.h" in (ROOT / "include" / "qsae_recycle.h").read_text()
    assert "qsae_recycle.h" in (ROOT / "quantizedsae_amd" / "build.py").read_text()


def test_calls_that_return_before_they_look_at_a_pointer():
    lib = _lib.load()
    flagged = _lib.C.c_int(7)
    # B == 0: QSAE_OK, nothing launched, the flagged-row count cleared
    assert lib.qsaer_binary_forward_prefilter(None, None, None, None, None, 0, 512, 8192, 16, None, 4, 1.0, None, None, None, None, 0,
                                              None, None, 0, 0, _lib.C.byref(flagged), None, None, 0) == _lib.OK
    assert flagged.value == 0
    assert lib.qsaer_table_forward_prefilter(None, None, None, None, None, 0, 512, 8192, 16, None, 1.0, None, None, None, None, 0,
                                             None, None, 0, 0, None, None, None, 0) == _lib.OK
    # the namesake's checks come first: a submit without a host word, a negative batch
    assert lib.qsaer_prefilter_submit(None, None, None, None, None, 4, 512, 8192, 16, None, 4, 1.0, None, None, None, None, 0, None,
                                      None, 0, None, None, None, 0) == _lib.ERR_INVALID_ARG
    assert b"qsaer_prefilter_submit" in lib.qsae_last_error()
    assert lib.qsaer_prefilter_submit_table(None, None, None, None, None, -1, 512, 8192, 16, None, 1.0, None, None, None, None, 0,
                                            None, None, 0, None, None, None, 0) == _lib.ERR_INVALID_ARG


# ---- the pool, on CPU tensors -----------------------------------------------------------------------------------------
KEY = ("cpu", 0, 4, 8, 2)


@pytest.fixture(autouse=True)
def empty_pool():
    ops.release_workspaces()
    yield
    ops.release_workspaces()


def _register(key=KEY):
    dense, idx = torch.zeros((key[2], key[3])), torch.zeros((key[2], key[4]), dtype=torch.int32)
    ops._latent_pool_register(key, dense, idx)
    return dense, idx


def _taken(key=KEY):
    return ops._latent_pool_take(key) is not None


def test_a_dropped_latent_is_taken_once_and_a_named_one_is_not():
    dense, idx = _register()
    hits, misses = ops.latent_pool_stats["hits"], ops.latent_pool_stats["misses"]
    assert not _taken()                                           # `dense` is still a name of it
    ptr = dense.data_ptr()
    del dense
    got = ops._latent_pool_take(KEY)
    assert got is not None and got[0].data_ptr() == ptr and got[1] is idx
    assert not _taken()                                           # the record left the pool with it
    assert (ops.latent_pool_stats["hits"], ops.latent_pool_stats["misses"]) == (hits + 1, misses + 2)
    _register()
    assert not _taken(KEY[:2] + (8, 8, 2)) and not _taken(KEY[:1] + (1,) + KEY[2:]) and _taken()     # another shape, another stream


HOLDERS = {
    "slice": lambda t: t[:, :7],
    "detached alias": lambda t: t.detach(),
    "numpy": lambda t: t.numpy(),
    "dlpack capsule": lambda t: torch.utils.dlpack.to_dlpack(t),
    "view kept in a list": lambda t: [t.view(-1)],
    "storage": lambda t: t.untyped_storage(),
}


@pytest.mark.parametrize("how", sorted(HOLDERS))
def test_whoever_still_holds_the_latent_keeps_it(how):
    dense, _ = _register()
    holder = HOLDERS[how](dense)
    del dense
    assert not _taken() and not _taken()
    del holder
    assert _taken()                                               # and it is free again once the holder is gone


def test_a_write_torch_sees_or_is_told_of_drops_the_record():
    dense, _ = _register()
    dense.add_(1)
    del dense
    assert not _taken() and not ops._latent_pool
    dense, idx = _register()
    idx.zero_()                                                   # the list no longer says what the latent holds
    del dense
    assert not _taken() and not ops._latent_pool
    dense, _ = _register()
    ops._latent_pool_forget(dense[1:])                            # by storage: any view of it will do
    del dense
    assert not ops._latent_pool and not _taken()
    keep, _ = _register()
    ops._latent_pool_forget(torch.zeros((4, 8)))                  # somebody else's tensor
    assert len(ops._latent_pool) == 1


def test_the_switch_the_bound_and_release_workspaces():
    assert ops.LATENT_RECYCLE is True and ops.LATENT_POOL_PER_DEVICE == 4
    first = [_register(("cpu", s, 4, 8, 2))[0].data_ptr() for s in range(6)]
    other = _register(("other device", 0, 4, 8, 2))[0].data_ptr()
    kept = [r.dense.data_ptr() for r in ops._latent_pool]
    assert kept == first[2:] + [other]                            # four per device, the oldest dropped first
    ops.release_workspaces()
    assert not ops._latent_pool and not _taken()


def test_two_threads_on_keys_of_their_own():
    rounds, errors = 300, []

    def worker(stream):
        key = ("cpu", stream, 4, 8, 2)
        try:
            held = None
            for i in range(rounds):
                got = ops._latent_pool_take(key)
                if i >= 2:
                    assert got is not None and got[0] is not held, (stream, i)      # the one dropped two rounds ago, never the held one
                    assert int(got[0][0, 0]) == stream and int(got[1][0, 0]) == i - 2
                dense = got[0] if got is not None else torch.empty((4, 8))
                got = None
                dense.fill_(float(stream))                                          # (before it is registered: not an edit)
                ops._latent_pool_register(key, dense, torch.full((4, 2), i, dtype=torch.int32))
                held, dense = dense, None                                           # keep the newest, drop the one before
        except Exception as e:                                                      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(s,)) for s in (1, 2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert {r.key[1] for r in ops._latent_pool} == {1, 2} and len(ops._latent_pool) <= 4
