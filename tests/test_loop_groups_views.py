"""dmx-demux-loop --groups --reorient --device-views (dmx/loop.py): the
operand table is built from a view run (pychopper's PASS segments as views of the raw batch, on
both strands), and the gene groups of every kept well still equal those dmx-similarity --groups
makes of the written well files; the files themselves do not change."""
import functools
import glob
import os
import subprocess

import numpy as np
import pytest

import operands_cases as oc
import test_loop_groups as lg
from helpers import LOOP, random_quals, write_fastq

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def raw_reads():
    """Raw reads for --reorient (pychopper's primers are the SP5 / SP27 adapters with N for the
    barcode): test_loop_groups' three wells of 96 (two gene families of 48 each, a few bodies
    below -min), a third stored reverse-complemented so that PASS views of both strands land in
    every well; then reads that are not PASS: 12 without a primer (no segment) and 12 fused ones
    (two segments), which reach no well."""
    rng = np.random.default_rng(31807)
    sp5, sp27 = lg._panels()
    tagged = []
    for w, (i, j) in enumerate(lg.WELLS):
        fams = [oc.rand_seq(rng, 360 + 40 * w), oc.rand_seq(rng, 430 + 25 * w)]
        for k in range(96):
            body = lg._mutate(rng, fams[k % 2], 0.03)
            if k % 17 == 0:
                body = body[:250]   # below -min 300: in the well, in no group
            tagged.append(oc.rand_seq(rng, rng.integers(0, 25)) + sp5[i].seq + body +
                          sp27[j].seq + oc.rand_seq(rng, rng.integers(0, 25)))
    n_pass = len(tagged)
    recs = [oc.revcomp(s) if rng.random() < 0.33 else s for s in tagged]
    recs += [oc.rand_seq(rng, rng.integers(300, 700)) for _ in range(12)]
    recs += [tagged[3 * k] + oc.revcomp(tagged[5 * k + 1]) for k in range(12)]
    order = rng.permutation(len(recs))
    seqs = [recs[k] for k in order]
    names = [f"raw{k} ch={k % 7}" for k in range(len(seqs))]
    return names, seqs, random_quals(rng, [len(s) for s in seqs]), n_pass


def _run(tmp_path, tag, *extra, check=True):
    d = tmp_path / tag
    d.mkdir(parents=True)
    infile = str(d / "s1.fastq.gz")
    write_fastq(infile, *raw_reads()[:3])
    out = d / "demuxed"
    r = subprocess.run([LOOP, "--reorient", infile, "-j", "4", "-q", "0.2", "--outdir", str(out),
                        *extra], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if check:
        assert r.returncode == 0, r.stderr[-3000:]
    return out, r


def test_groups_of_a_view_run_equal_dmx_similarity_on_the_well_files(tmp_path):
    g = tmp_path / "groups.tsv"
    out, _ = _run(tmp_path, "with", "--device-views", "--groups", str(g))
    plain, _ = _run(tmp_path, "without", "--device-views")
    files = sorted(os.path.relpath(p, out) for p in glob.glob(str(out / "SP*" / "*.fastq.gz")))
    assert files == sorted(os.path.relpath(p, plain)
                           for p in glob.glob(str(plain / "SP*" / "*.fastq.gz")))
    assert len(files) > len(lg.WELLS)
    for f in files:   # the outputs the loop writes without --groups are unchanged
        assert (out / f).read_bytes() == (plain / f).read_bytes(), f
    # the PASS records alone were demultiplexed: reads without a segment or with two are not PASS
    n_pass = raw_reads()[3]
    pych = tmp_path / "with" / "pychopped"
    text = (pych / "s1_pass.fastq").read_text()
    assert text.count("\n+\n") == n_pass and "strand=-" in text and "strand=+" in text
    lg.groups_equal_dmx_similarity(tmp_path, out, g, "s1")


def test_groups_with_reorient_need_device_views(tmp_path):
    g = tmp_path / "groups.tsv"
    _, r = _run(tmp_path, "host", "--groups", str(g), check=False)
    assert r.returncode == 2 and not g.exists()
    assert "--groups with --reorient needs --device-views" in r.stderr
