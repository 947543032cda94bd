"""The example's --sam flag (fmindex-collection_amd/example/main.cpp): under --mode map the --save_output file is a SAM file, the header (fmgpu_sam_header) followed by
the records made on the device (fmgpu_positions_sam through fmc::formatSam); the records equal format_sam of the positions the plain run reports.  Without --mode map,
with --packed or with --device-format the flag is refused."""
import subprocess

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd.capi import POSITION_DTYPE
from tests.test_example_cli import EXE, _fasta, load_fasta
from tests.test_example_cli_parse import _build, _run, _stable


def test_help_names_the_flag_and_it_needs_mode_map(tmp_path):
    _build()
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--sam" in r.stdout
    for extra in ([], ["--mode", "besthits"], ["--mode", "map", "--packed"], ["--mode", "map", "--device-format"]):
        r = subprocess.run([EXE, "--index", str(tmp_path / "none.fasta"), "--query", str(tmp_path / "none.fasta"), "--sam"] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "--sam needs --mode map" in r.stderr


@pytest.mark.gpu
def test_sam_records_equal_format_sam_of_the_plain_positions(tmp_path):
    _build()
    rng = np.random.default_rng(23)
    ref, qry, rp, qp = _fasta(rng, tmp_path)
    lengths = [len(s) for s in load_fasta(ref, False)]
    header = fm.sam_header(["chrA", "chrB", "chrC"], lengths, "fmindex-collection-gpu-example")
    assert header.count(b"@SQ") == 3
    ladder = ["--algo", "ng26", "--gen", "h2-k2", "--min_k", "2", "--max_k", "2", "--mode", "map"]
    exact = ["--algo", "noerror", "--min_k", "0", "--max_k", "0", "--mode", "map"]
    for flags in (ladder, exact):
        for extra in ([], ["--feed"], ["--feed", "--device-parse", "--pair-strands"]):
            plain, rows = _run(rp, qp, str(tmp_path / "plain.txt"), flags, extra)
            assert plain.returncode == 0 and len(rows) > 0, (flags, extra, plain.stdout + plain.stderr)
            r, got = _run(rp, qp, str(tmp_path / "out.sam"), flags, extra + ["--sam"])
            assert r.returncode == 0, (flags, extra, r.stdout + r.stderr)
            assert _stable(r.stdout) == _stable(plain.stdout), (flags, extra)
            positions = np.array([tuple(int(v) for v in ln.split()) + (0,) for ln in rows.decode().splitlines()], dtype=POSITION_DTYPE)
            pair = "--pair-strands" in extra
            batch = [np.array(q, dtype=np.uint8) for q in load_fasta(qry, not pair)]       # the searched batch: with its reverse complements unless the device makes them
            want = fm.format_sam(positions, batch, strands=[0, 4, 3, 2, 1, 5] if pair else None, seq_names=[b"chrA first", b"chrB", b"chrC lower case"],
                                 cigar=flags is exact)
            assert got == header + want, (flags, extra)
            records = [ln.split(b"\t") for ln in got[len(header):].splitlines()]
            assert sum(1 for f in records if not int(f[1]) & 4) == len(positions) and len(records) >= len(batch)
            assert any(int(f[1]) & 16 for f in records) == pair
