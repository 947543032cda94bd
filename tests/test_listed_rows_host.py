"""The delimiter-row lists of Formats P and D on the CPU (tests/listed_rows_model.py on the collections of tests/listed_rows_cases.py): the model with the corrections
returns the intervals, miss rows and step counts of a plain backward search and of the oracle on every read; the model WITHOUT them returns something else on a stated
share of every read family — so a device kernel whose correction were wrong by a few rows could not pass tests/test_gpu_listed_rows.py, which compares the same reads with
the same oracle — and the reads meet the listed rows the way the coverage conditions ask (many in one line, ends on listed rows, the lists' last slots)."""
import numpy as np
import pytest

import fmindex_collection_amd as fm
from tests import listed_rows_cases as cases
from tests.listed_rows_model import ListedRows, _String, plain_search


def test_model_tables_on_a_hand_made_bwt():
    """pair_rank and dense_rank against their definitions, row by row, on a text with empty, one-symbol and repeated sequences"""
    seqs = [[1, 1, 2], [], [1], [1, 1, 2], [3, 1, 1, 1, 4], [], [2]]
    ox = cases.fo.OraIndex.build("IB16", 5, [np.array(s, dtype=np.uint8) for s in seqs], 1, True)
    bwt, rev = cases.bwt_of(ox.bwt_string()), cases.bwt_of(ox.bwt_string(rev=True))
    mo = ListedRows(bwt, rev)
    assert len(mo.pairs_ex) == 2 * 5 + 2 and len(mo.dense[0]["ex"]) == 7 and len(mo.dense[1]["ex"]) == 7      # two per non-empty sequence, one per empty one; one per sequence
    s = _String(bwt)
    lf = s.lf_rows()
    for i in range(mo.n + 1):
        for pc in range(16):
            x, y = (pc >> 2) + 1, (pc & 3) + 1
            assert mo.pair_rank(i, pc) == s.lf(s.lf(i, y), x), (i, pc)                                       # LF_x(LF_y(i)): "xy" prepended in one step
            assert mo.pair_rank(i, pc) == s.lf(s.lf(0, y), x) + sum(1 for j in range(i) if bwt[j] == y and bwt[lf[j]] == x)
        for c in range(1, 5):
            assert mo.dense_rank(i, c) == s.lf(i, c) and mo.dense_rank(i, c, rev=True) == _String(rev).lf(i, c)
    assert [mo.row_symbol(i) for i in range(mo.n)] == [int(v) for v in bwt] and [mo.row_symbol(i, True) for i in range(mo.n)] == [int(v) for v in rev]
    off = ListedRows(bwt, rev, corrections=False)
    assert all(off.row_symbol(i) == 1 for i in mo.dense[0]["ex"]) and off.pair_rank(mo.n, 0) == mo.pair_rank(mo.n, 0) + mo.listed_before(mo.n)
    # the filter: a line is flagged by its own listed rows and by those of every line `bits` lines away
    small = ListedRows(bwt, rev, bits=1)
    small.pair_rank(3, 0)
    assert small.pair_events()["flagged"].all() and mo.pair_flag.sum() == len(set(int(v) >> 7 for v in mo.pairs_ex))


@pytest.mark.parametrize("name", cases.SMALL)
def test_model_with_corrections_equals_plain_search_and_oracle(name):
    w, mo = cases.walk(name), cases.model(name)
    reads = w["reads"]
    qbuf, qoff = fm.flatten(list(reads))
    olb, oln, ost = cases.oracle(name, True).search_exact(qbuf, qoff, want_steps=True)
    for i, r in enumerate(reads):
        want = (int(olb[i]), int(oln[i]), int(ost[i]))
        assert w["fixed"]["pairs"][i] == want == plain_search(mo.fw, r), (name, i, w["label"][i])
    for i in w["clean"]:
        assert w["fixed"]["dense"][False][i] == (int(olb[i]), int(oln[i]), int(ost[i])), (name, i)
        assert w["fixed"]["dense"][True][i] == plain_search(mo.rv, reads[i][::-1]), (name, i)
        assert w["fixed"]["dense"][True][i][1] == int(oln[i])


# the share of a family's reads on which the model without the lists must return another interval (lb or len) than the model with them: Format P in pair steps,
# Format D in one-symbol steps forward (bwt) and in the other direction (bwtRev).  None: the family does not show it there, and cannot —
#   an overhang BEHIND a sequence's end is appended across a delimiter row of bwtRev: only the other direction of Format D prepends across one;
#   "A", "AAA", "CA", "AC" in front are taken by the pair steps with the delimiter in a pair that is not "AA" (or, "A": only where the sequence starts with 'A');
#   "AC" in front and "CA" behind meet the delimiter row with a 'C' step, which no list corrects.
SHARES = {"windows": (0.25, 0.25, 0.25), "thresholds": (0.25, 0.25, 0.25), "whole": (0.5, 0.5, 0.5), "a_runs": (0.1, None, None), "cluster": (0.4, None, None),
          "overhang_front:A": (None, 0.9, None), "overhang_front:AA": (0.9, 0.9, None), "overhang_front:AAA": (None, 0.9, None), "overhang_front:CA": (None, 0.8, None),
          "overhang_front:AC": (None, None, None),
          "overhang_behind:A": (None, None, 0.9), "overhang_behind:AA": (None, None, 0.9), "overhang_behind:AAA": (None, None, 0.9), "overhang_behind:CA": (None, None, None),
          "overhang_behind:AC": (None, None, 0.8)}


@pytest.mark.parametrize("name", cases.SMALL)
def test_model_without_corrections_is_caught_on_every_family(name):
    w = cases.walk(name)
    shown = set()
    for f in cases.FAMILIES:
        idx = [i for i, l in enumerate(w["label"]) if l == f]
        if not idx:
            assert f == "cluster" and name != "clustered"            # (the family of the collection with copies of one sequence)
            continue
        clean = [i for i in idx if i in w["fixed"]["dense"][False]]
        got = (sum(w["fixed"]["pairs"][i][:2] != w["broken"]["pairs"][i][:2] for i in idx) / len(idx),
               sum(w["fixed"]["dense"][False][i][:2] != w["broken"]["dense"][False][i][:2] for i in clean) / max(1, len(clean)),
               sum(w["fixed"]["dense"][True][i][:2] != w["broken"]["dense"][True][i][:2] for i in clean) / max(1, len(clean)))
        print(name, f, len(idx), "P %.2f  D %.2f  D other direction %.2f" % got)
        for share, floor in zip(got, SHARES[f]):
            if floor is not None:
                assert share >= floor, (name, f, got)
                shown.add(f)
    assert set(cases.FAMILIES) - shown <= {"overhang_front:AC", "overhang_behind:CA", "cluster"}


@pytest.mark.parametrize("name", cases.SMALL)
def test_reads_meet_the_coverage_conditions(name):
    w = cases.walk(name)
    ev = w["events_p"]
    c = ev["correction"]
    print(name, "AA ends", len(c), "correction >= 1 / 8 / 64:", int((c >= 1).sum()), int((c >= 8).sum()), int((c >= 64).sum()), "on a listed row", int(ev["on_listed"].sum()),
          "first row of a flagged line", int(((ev["row"] & 127 == 0) & ev["flagged"]).sum()))
    for rev in (False, True):
        c = w["events_d"][rev]["correction"]
        print(name, "A ends, bwtRev" if rev else "A ends, bwt", len(c), "correction >= 1 / 8:", int((c >= 1).sum()), int((c >= 8).sum()))
    if name == "clustered":
        print(name, "overhang reads that hit without the lists (of those that can):", cases.overhang_hits_without_corrections(name))
    cases.check_coverage(name)


def test_the_lists_stand_at_and_past_their_caps():
    sizes = {name: (len(cases.model(name).pairs_ex), len(cases.model(name).dense[0]["ex"]), len(cases.model(name).dense[1]["ex"])) for name in cases.SMALL}
    assert sizes["cap"] == (512, 256, 256) and sizes["cap+1"] == (514, 257, 257) and sizes["mixed"] == (457, 257, 257)
    assert sizes["clustered"][1:] == (256, 256) and 480 <= sizes["clustered"][0] <= 512
    mo = cases.model("clustered")
    assert np.bincount(mo.pairs_ex >> 7).max() >= 120 and np.bincount(mo.dense[0]["ex"] >> 6).max() == 64      # a line of listed rows, a block of delimiter rows
    assert all(cases.model(name).n < 200_000 for name in cases.SMALL)


@pytest.mark.parametrize("length", [31, 64])
@pytest.mark.parametrize("name", cases.SMALL)
def test_lean_overhang_reads_stand_on_delimiter_rows(name, length):
    """the equal-length batches: behind the 'A's in front of a sequence's first symbols the walk stands on rows of bwt that hold the delimiter (one row, or the run of
    the copies), and in front of the 'A's behind its last symbols on such rows of bwtRev — what a_is_delim and delims_before are there for"""
    mo = cases.model(name)
    stood = [0, 0]
    for r in cases.lean_reads(name, length, 1):
        for rev in (False, True):
            for a in (1, 2, 3):
                if not (r[-a:] if rev else r[:a]).tolist() == [1] * a:
                    break
                lb, ln, _ = mo.search_dense(r[:-a] if rev else r[a:], rev)
                ex = mo.dense[int(rev)]["ex"]
                if ln and np.searchsorted(ex, lb + ln) - np.searchsorted(ex, lb) == ln:
                    stood[int(rev)] += 1
                    assert all(mo.row_symbol(i, rev) == 0 for i in range(lb, lb + ln))
                    break
    print(name, length, "reads that stand on delimiter rows of bwt / bwtRev:", stood)
    assert min(stood) >= 20
