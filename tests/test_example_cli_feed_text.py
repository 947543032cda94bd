"""The example with --mode map --feed --device-parse and reverse complements off (fmindex-collection_amd/example/main.cpp): the bytes of the query file go through
fmc::Feed::mapText (fmgpu_feed_map_text), and the --save_output file is the one the same run writes without --device-parse, for a FASTA and for a FASTQ query file."""
import numpy as np
import pytest

from tests.test_example_cli import _fasta
from tests.test_example_cli_parse import _build, _run, _stable


@pytest.mark.gpu
def test_text_through_the_feed_writes_the_same_output(tmp_path):
    _build()
    rng = np.random.default_rng(29)
    ref, qry, rp, qp = _fasta(rng, tmp_path)
    reads = [ln for ln in qry.split("\n") if ln and not ln.startswith(">")]
    fq = tmp_path / "reads.fastq"
    fq.write_text("".join("@read%d\n%s\n+\n%s\n" % (i, r, "".join(chr(33 + (i + k) % 41) for k in range(len(r)))) for i, r in enumerate(reads)))
    base = ["--mode", "map", "--feed", "--no-reverse"]
    for flags in (["--algo", "noerror", "--min_k", "0", "--max_k", "0"], ["--algo", "ng26", "--gen", "h2-k2", "--min_k", "0", "--max_k", "2", "--stepSize_k", "2"]):
        out = str(tmp_path / "out.txt")
        plain, saved = _run(rp, qp, out, base + flags, [])
        assert plain.returncode == 0 and len(saved) > 0, (flags, plain.stdout + plain.stderr)
        for path in (qp, str(fq)):
            r, got = _run(rp, path, out, base + flags, ["--device-parse"])
            assert r.returncode == 0, (flags, path, r.stdout + r.stderr)
            assert "bytes of query text" in r.stdout                                  # the text path ran: no read was a vector on the host
            assert got == saved, (flags, path)
            assert [ln for ln in _stable(r.stdout) if not ln.startswith("loaded ")] == [ln for ln in _stable(plain.stdout) if not ln.startswith("loaded ")]
    # with reverse complements on, today's path stays
    r, got = _run(rp, qp, str(tmp_path / "both.txt"), ["--mode", "map", "--feed", "--algo", "noerror", "--min_k", "0", "--max_k", "0"], ["--device-parse"])
    assert r.returncode == 0 and "incl reverse complements" in r.stdout and "bytes of query text" not in r.stdout and len(got) > 0
