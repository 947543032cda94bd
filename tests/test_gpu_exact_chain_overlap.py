"""Exact search along the sample chain, the two legs between park and resume: the jump over all reads (the reads the park launch parked) on the caller's stream, the continue
launch and the jump over its list (the reads it parked late) on the library's side stream.  Both jumps read the query from the register window.  Intervals, miss rows and
the step count equal the oracle's one-symbol search; the serial order (FMGPU_DEV_EXACT_SERIAL, development build) gives the same bytes and the same stats; two calls of one
thread on two streams do not disturb each other; list lengths 0, 1 and "every read"."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from tests.test_gpu_sample_chain import STAT_FIELDS, expected, make, oracle, reads, sequences

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIQUE = 60_000           # sequences()[0][:UNIQUE] is random text; [UNIQUE, UNIQUE + 20 000) is the block the text holds three times
BLOCK = 20_000


def stats_of(st):
    return tuple(int(getattr(st, f)) for f in STAT_FIELDS)


@functools.lru_cache(maxsize=None)
def index(rate):
    return make(rate, "arrays")


def waves_of(long_reads, blocks, seed):
    """whole waves: in every block of 64 reads 56 copies of 5 symbols and 8 of long_reads(rng), the long ones at lanes of their own in every block"""
    s = sequences()[0]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(blocks):
        lanes = set(rng.choice(64, size=8, replace=False).tolist())
        for lane in range(64):
            if lane in lanes:
                out.append(long_reads(rng))
            else:
                p = int(rng.integers(0, UNIQUE - 5))
                out.append(s[p: p + 5].copy())
    return fm.flatten(out)


@functools.lru_cache(maxsize=None)
def late_batch():
    """the short reads end after two pair passes, the long ones (160 symbols of unique text) still hold many rows then: the wave hands its 8 live lanes over, the continue
    launch parks them, and every jump of the batch happens in the jump over the list"""
    s = sequences()[0]

    def long_read(rng):
        p = int(rng.integers(0, UNIQUE - 160))
        return s[p: p + 160].copy()
    return waves_of(long_read, 32, 41)


@functools.lru_cache(maxsize=None)
def repeat_batch():
    """as late_batch, the long reads from inside the repeated block: they never reach one row, so every one of them is listed and none is ever parked"""
    s = sequences()[0]

    def long_read(rng):
        m = (101, 128, 160)[int(rng.integers(0, 3))]
        p = UNIQUE + int(rng.integers(0, BLOCK - m))
        return s[p: p + m].copy()
    return waves_of(long_read, 16, 43)


@functools.lru_cache(maxsize=None)
def want(batch):
    qbuf, qoff = batch()
    return oracle(16).search_exact(qbuf, qoff, want_steps=True)


def tail(batch, k):
    """the batch of every read's last k symbols (what a backward search has consumed after k steps)"""
    qbuf, qoff = batch
    return fm.flatten([qbuf[max(int(qoff[i]), int(qoff[i + 1]) - k): qoff[i + 1]] for i in range(len(qoff) - 1)])


def check(gx, batch, olb, oln, ost, rate, packed=False):
    q = fm.pack_queries(batch, 5) if packed else batch
    lb, ln, st = fm.search_no_errors.search(gx, q, want_stats=True)
    print("rate", rate, "packed", packed, "reads", len(oln), "lf_steps", st.lf_steps, "oracle", int(ost.sum()), "table_steps", st.table_steps,
          "wrong lb", int((lb != olb).sum()), "wrong len", int((ln != oln).sum()))
    assert np.array_equal(ln, oln) and np.array_equal(lb, olb)
    assert st.lf_steps == int(ost.sum())
    assert st.table_steps % rate == 0
    return st


def test_late_batch_is_what_it_claims():
    """on the CPU, with the oracle: after 4 symbols a long read still holds more than one row, and it is one row while at least 32 symbols remain"""
    batch = late_batch()
    qbuf, qoff = batch
    long_ = np.flatnonzero(np.diff(qoff.astype(np.int64)) == 160)
    assert len(long_) == 32 * 8 and all(len(set((long_[8 * b: 8 * b + 8] // 64).tolist())) == 1 for b in range(32))
    _, len4 = oracle(16).search_exact(*tail(batch, 4))
    _, len128 = oracle(16).search_exact(*tail(batch, 128))
    assert (len4[long_] > 1).all() and (len128[long_] == 1).all()


@pytest.mark.parametrize("rate", [1, 4, 16])
def test_late_parks_go_through_the_list_jump(rate):
    olb, oln, ost = want(late_batch)
    st = check(index(rate), late_batch(), olb, oln, ost, rate)
    assert st.table_steps > 0
    st4 = check(index(rate), late_batch(), olb, oln, ost, rate, packed=True)
    assert stats_of(st4) == stats_of(st)


@pytest.mark.parametrize("rate", [4, 16])
def test_both_legs_in_one_call(rate):
    """the mixed batch (reads the park launch parks, reads the continue launch parks, lengths 145 / 160 / 300 that refill the window), byte form and 4-bit form"""
    olb, oln, ost = expected()
    st = check(index(rate), reads(), olb, oln, ost, rate)
    st4 = check(index(rate), reads(), olb, oln, ost, rate, packed=True)
    assert st.table_steps > 0 and stats_of(st4) == stats_of(st)


_SERIAL_PROBE = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "oracle"))
import numpy as np
import fmindex_collection_amd as fm
from tests.test_gpu_sample_chain import make, reads
from tests.test_gpu_exact_chain_overlap import late_batch, stats_of
out = {}
for rate in (4, 16):
    gx = make(rate, "built")
    for name, batch in (("late", late_batch()), ("mixed", reads())):
        for form in ("bytes", "q4"):
            q = fm.pack_queries(batch, 5) if form == "q4" else batch
            os.environ.pop("FMGPU_DEV_EXACT_SERIAL", None)
            a = fm.search_no_errors.search(gx, q, want_stats=True)
            os.environ["FMGPU_DEV_EXACT_SERIAL"] = "1"
            b = fm.search_no_errors.search(gx, q, want_stats=True)
            os.environ.pop("FMGPU_DEV_EXACT_SERIAL", None)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (rate, name, form)
            assert stats_of(a[2]) == stats_of(b[2]) and a[2].table_steps > 0, (rate, name, form, stats_of(a[2]), stats_of(b[2]))
            out["%%s_%%d_%%s_lb" %% (name, rate, form)] = b[0]; out["%%s_%%d_%%s_len" %% (name, rate, form)] = b[1]
            out["%%s_%%d_%%s_steps" %% (name, rate, form)] = np.array([b[2].lf_steps], dtype=np.uint64)
np.savez(sys.argv[1], **out)
print("SERIAL_EQUAL", len(out))
"""


def test_serial_equals_overlapped(tmp_path):
    """the development build reads FMGPU_DEV_EXACT_SERIAL at every call: all five launches on the caller's stream.  One child process (the library is chosen at import)
    runs both batches, both rates and both query forms with and without the knob and compares the bytes and every field of the stats; its serial results equal the oracle here."""
    dev_lib = os.path.join(ROOT, "fmindex-collection_amd", "libfmgpu_dev.so")
    assert os.path.exists(dev_lib), "libfmgpu_dev.so is not built (make -C fmindex-collection_amd/csrc DEV=1)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FMGPU_")}
    env["FMGPU_LIBRARY"] = dev_lib
    path = str(tmp_path / "serial.npz")
    r = subprocess.run([sys.executable, "-c", _SERIAL_PROBE % (ROOT, ROOT), path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "SERIAL_EQUAL 24" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(path)
    for name, (olb, oln, ost) in (("late", want(late_batch)), ("mixed", expected())):
        for rate in (4, 16):
            for form in ("bytes", "q4"):
                key = "%s_%d_%s_" % (name, rate, form)
                assert np.array_equal(got[key + "lb"], olb) and np.array_equal(got[key + "len"], oln) and int(got[key + "steps"][0]) == int(ost.sum()), key


def test_two_calls_on_two_streams():
    """one handle, one thread, two streams, the second call issued while the first one's kernels may still run: the second call waits for the event recorded behind the first
    one's last kernel (after the side stream's join) before it touches the state the two share"""
    import torch
    gx = index(16)
    L = capi.lib()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    jobs = []
    for batch, exp, stream in ((reads(), expected(), s1), (late_batch(), want(late_batch), s2)):
        qbuf, qoff = batch
        nq = len(qoff) - 1
        jobs.append((fm.DeviceBuffer.from_array(qbuf), fm.DeviceBuffer.from_array(qoff), nq, fm.DeviceBuffer(8 * nq), fm.DeviceBuffer(8 * nq), exp, stream))
    for rnd in range(3):
        for dq, do, nq, dlb, dln, _, stream in jobs:
            capi.check(L.fmgpu_search_exact(gx._h, capi.ptr(dq), capi.ptr(do), nq, capi.ptr(dlb), capi.ptr(dln), None, C.c_void_p(stream.cuda_stream)))
        torch.cuda.synchronize()
        for dq, do, nq, dlb, dln, (olb, oln, _), _ in jobs:
            lb, ln = dlb.to_array(np.uint64, nq), dln.to_array(np.uint64, nq)
            assert np.array_equal(ln, oln) and np.array_equal(lb, olb), rnd
            junk = np.full(nq, 0xabababababababab, dtype=np.uint64)
            capi.check(L.fmgpu_memcpy_h2d(capi.ptr(dlb), capi.ptr(junk), 8 * nq))
    for job in jobs:
        for b in job[:2] + job[3:5]:
            b.free()


@pytest.mark.parametrize("nq", [1, 63, 65])
def test_list_form_edge_sizes(nq):
    """a last wave of one lane, of 63, and one lane into the second wave: the first reads of the mixed batch and of the batch whose every jump is in the list"""
    gx = index(16)
    for batch, (olb, oln, ost) in ((reads(), expected()), (late_batch(), want(late_batch))):
        qbuf, qoff = batch
        part = (qbuf[: qoff[nq]], qoff[: nq + 1])
        check(gx, part, olb[:nq], oln[:nq], ost[:nq], 16)
        check(gx, part, olb[:nq], oln[:nq], ost[:nq], 16, packed=True)


@pytest.mark.parametrize("how", ["distinct", "same_per_wave"])
def test_empty_list(how):
    """every read is 64 symbols of unique text.  same_per_wave: the 64 lanes of a wave hold one read, so they all park in one pass, no wave ever has 1..10 live lanes and the
    list is empty for certain (continue and the jump over the list return at once); distinct: 64 different reads per wave, whose last lanes may still be handed over"""
    s = sequences()[0]
    rng = np.random.default_rng(47)
    starts = rng.integers(0, UNIQUE - 64, size=16 if how == "same_per_wave" else 1024)
    batch = fm.flatten([s[p: p + 64].copy() for p in (np.repeat(starts, 64) if how == "same_per_wave" else starts)])
    olb, oln, ost = oracle(16).search_exact(*batch, want_steps=True)
    assert (oln == 1).all()
    st = check(index(16), batch, olb, oln, ost, 16)
    assert st.table_steps > 0


def test_every_long_read_listed_none_parked():
    """reads from inside the block the text holds three times never reach one row: as the last live lanes of their waves they are all listed, none is parked by either
    launch, and both jumps find nothing to do"""
    olb, oln, ost = want(repeat_batch)
    qbuf, qoff = repeat_batch()
    assert (oln[np.diff(qoff.astype(np.int64)) > 5] >= 3).all()
    st = check(index(16), repeat_batch(), olb, oln, ost, 16)
    assert st.table_steps == 0
    # ... and a batch of eight such reads alone: the whole batch is the list from the first pass on
    long_ = np.flatnonzero(np.diff(qoff.astype(np.int64)) > 5)[:8]
    few = fm.flatten([qbuf[qoff[i]: qoff[i + 1]] for i in long_])
    st = check(index(16), few, olb[long_], oln[long_], ost[long_], 16)
    assert st.table_steps == 0
