"""`dmx-demux-loop --reorient --device-views`: the PASS segments stay on the
GPU as views of the resident raw batch.  Every file it writes must be byte-identical to
`--reorient` without the flag: the demultiplexed bins, pychopper's five outputs, the JSON
reports (but for the command line they record), and the statistics printed at the end."""
import glob
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

from dmx import synth
from helpers import LOOP, write_fastq

pytestmark = pytest.mark.gpu


def _records(rng, n):
    """tests/test_chop.py's raw reads: both strands, fused reads, cut reads, N runs, and a tenth
    with qualities under -Q 10."""
    d = synth.generate("c2", n=n, seed=int(rng.integers(1 << 30)))
    seqs = []
    for s in synth.to_strings(d):
        u = rng.random()
        if u < 0.10 and seqs:
            s = s + seqs[-1]
        elif u < 0.15:
            s = s[:int(rng.integers(0, 130))]
        elif u < 0.20:
            p = int(rng.integers(0, len(s)))
            s = s[:p] + "N" * int(rng.integers(1, 6)) + s[p:]
        seqs.append(s)
    quals = []
    for s in seqs:
        lo, hi = (2, 14) if rng.random() < 0.1 else (5, 41)
        quals.append("".join(chr(33 + int(x)) for x in rng.integers(lo, hi, size=len(s))))
    return [f"r{i} runid=abc ch={i % 512}" for i in range(n)], seqs, quals


def _stats_lines(text):
    """The loop's printed statistics without its timing and path lines."""
    keep = [ln for ln in text.splitlines()
            if not re.match(r"(Processing|Output directory|Results in|Finished in)", ln)]
    return keep


@pytest.mark.parametrize("q,extra", [("0.2", []), (None, ["--no-cleanup"])])
def test_device_views_writes_the_same_files(tmp_path, q, extra):
    names, seqs, quals = _records(np.random.default_rng(61), 600)
    outs = {}
    for tag, flag in (("host", []), ("dev", ["--device-views"])):
        d = tmp_path / tag
        d.mkdir()
        write_fastq(str(d / "sample.fastq.gz"), names, seqs, quals)
        cmd = [LOOP, "--reorient", str(d / "sample.fastq.gz"), "-j", "4", "--batch-mb", "1",
               "--device", "0"] + flag + extra + (["-q", q] if q else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[tag] = _stats_lines(r.stdout)
    assert outs["host"] == outs["dev"]
    host, dev = tmp_path / "host", tmp_path / "dev"
    for k in ("pass", "rescued", "unclass", "short"):
        a = (host / "pychopped" / f"sample_{k}.fastq").read_bytes()
        assert a == (dev / "pychopped" / f"sample_{k}.fastq").read_bytes(), k
    assert (host / "pychopped" / "sample_stats.out").read_text() == \
        (dev / "pychopped" / "sample_stats.out").read_text()
    files = sorted(os.path.relpath(p, host / "demuxed")
                   for p in glob.glob(str(host / "demuxed" / "*" / "*")))
    assert files == sorted(os.path.relpath(p, dev / "demuxed")
                           for p in glob.glob(str(dev / "demuxed" / "*" / "*")))
    assert sum(f.endswith(".fastq.gz") for f in files) >= 12 + 12 * 8
    n_rec = n_json = 0
    for f in files:
        a, b = host / "demuxed" / f, dev / "demuxed" / f
        if f.endswith(".gz"):
            assert a.read_bytes() == b.read_bytes(), f
            n_rec += gzip.decompress(a.read_bytes()).count(b"\n+\n")
        else:
            ja, jb = json.loads(a.read_text()), json.loads(b.read_text())
            for j in (ja, jb):
                assert "--reorient" in j["command_line_arguments"]
                j.pop("command_line_arguments")       # the flag itself
                j.pop("input")                        # the two runs' directories
            assert ja == jb, f
            n_json += 1
    assert n_rec > 0.4 * len(seqs)
    assert n_json == 1 + 12       # the round-1 report and one round-2 report per SP5 bin


def test_device_views_needs_reorient(tmp_path):
    f = tmp_path / "x.fastq"
    f.write_text("")
    r = subprocess.run([LOOP, str(f), "--device-views"], capture_output=True, text=True)
    assert r.returncode == 2 and "--device-views goes with --reorient" in r.stderr
