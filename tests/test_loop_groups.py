"""dmx-demux-loop --groups (dmx/loop.py): the gene groups of every kept well
from the resident reads equal those dmx-similarity --groups makes of the written well files, the
files themselves do not change, and an input of two batches is refused before FILE exists."""
import functools
import glob
import os
import subprocess

import numpy as np
import pytest

import operands_cases as oc
from dmx import panel, sorter
from helpers import LOOP, random_quals, read_fastq, write_fastq

pytestmark = pytest.mark.gpu
SIM = os.path.join(os.path.dirname(LOOP), "dmx-similarity")
WELLS = ((0, 0), (1, 2), (0, 1))   # (SP5, SP27) adapter indices of the three kept wells


def _panels():
    a, b = panel.AdapterSet(), panel.AdapterSet()
    a.add_spec(f"file:{panel.SP5_FASTA}", "front")
    b.add_spec(f"file:{panel.SP27RC_FASTA}", "back")
    return a.adapters, b.adapters


def _mutate(rng, s, rate):
    s = list(s)
    for i in range(len(s)):
        if rng.random() < rate:
            s[i] = "ACGT"[int(rng.integers(4))]
    return "".join(s)


@functools.lru_cache(maxsize=None)
def reads():
    """300 reads: three wells of 96 (two gene families each, a third of the reads stored
    reverse-complemented, a few bodies below -min), one SP27_010 read, and 11 reads without
    adapters that are long enough to push the input over a 1 MB batch."""
    rng = np.random.default_rng(31804)
    sp5, sp27 = _panels()
    assert sp27[9].name == "SP27_010"
    out = []
    for w, (i, j) in enumerate(WELLS):
        fams = [oc.rand_seq(rng, 360 + 40 * w), oc.rand_seq(rng, 430 + 25 * w)]
        for k in range(96):
            body = _mutate(rng, fams[k % 2], 0.03)
            if k % 17 == 0:
                body = body[:250]   # below -min 300: in the well, in no group
            out.append((i, j, body))
    out.append((2, 9, oc.rand_seq(rng, 400)))
    recs = []
    for i, j, body in out:
        s = (oc.rand_seq(rng, rng.integers(0, 25)) + sp5[i].seq + body + sp27[j].seq +
             oc.rand_seq(rng, rng.integers(0, 25)))
        recs.append(oc.revcomp(s) if rng.random() < 0.33 else s)
    recs += [oc.rand_seq(rng, 60000) for _ in range(11)]
    order = rng.permutation(len(recs))
    seqs = [recs[k] for k in order]
    assert len(seqs) == 300
    names = [f"read{k} ch={k % 7}" for k in range(len(seqs))]
    return names, seqs, random_quals(rng, [len(s) for s in seqs])


def _run(tmp_path, tag, *extra, check=True):
    d = tmp_path / tag / "pychopped"
    d.mkdir(parents=True)
    infile = str(d / "pychopped_s1.fastq.gz")
    write_fastq(infile, *reads())
    out = tmp_path / tag / "demuxed"
    r = subprocess.run([LOOP, infile, "-j", "4", "--outdir", str(out), *extra],
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if check:
        assert r.returncode == 0, r.stderr
    return out, r


def groups_equal_dmx_similarity(tmp_path, out, g, ds):
    """FILE g of a --groups run into `out` names the kept wells of dataset `ds` in file-name
    order, every read of a well in the well file's order, and per well the groups that
    dmx-similarity --groups makes of the written well file."""
    rows = [ln.split("\t") for ln in g.read_text().splitlines()]
    wells = sorted({r[0] for r in rows})
    sp5, sp27 = _panels()
    assert wells == sorted(f"{sp27[j].name}_{sp5[i].name}_{ds}.fastq.gz" for i, j in WELLS)
    assert [r[0] for r in rows] == sorted(r[0] for r in rows)   # wells in file-name order
    for w in wells:
        path = str(out / "SP27" / w)
        recs = read_fastq(path)
        ids = [r[0].split()[0].lstrip("@") for r in recs]
        mine = [r for r in rows if r[0] == w]
        assert [r[1] for r in mine] == ids and len(ids) >= 90   # every read, in input order
        by_label = {}
        for _, rid, lab in mine:
            if lab != "-":
                by_label.setdefault(lab, set()).add(rid)
        got = {frozenset(v) for v in by_label.values()}
        gf = tmp_path / (w + ".groups")
        subprocess.run([SIM, "-i", path, "--groups", str(gf)], check=True,
                       stderr=subprocess.DEVNULL)
        kept = sorter.usable([len(r[1]) for r in recs], 300, None)
        exp = {frozenset(ids[int(kept[int(x)])] for x in ln.split())
               for ln in gf.read_text().splitlines() if ln.strip()}
        assert got == exp and len(exp) >= 2 and sum(len(x) for x in exp) >= 80
        assert any(lab == "-" for _, _, lab in mine)   # the short records are in no group


def test_groups_equal_dmx_similarity_on_the_well_files(tmp_path):
    g = tmp_path / "groups.tsv"
    out, _ = _run(tmp_path, "with", "--groups", str(g))
    plain, _ = _run(tmp_path, "without")
    files = sorted(os.path.relpath(p, out) for p in glob.glob(str(out / "SP*" / "*.fastq.gz")))
    assert files == sorted(os.path.relpath(p, plain)
                           for p in glob.glob(str(plain / "SP*" / "*.fastq.gz")))
    for f in files:   # the outputs the loop writes today are unchanged
        assert (out / f).read_bytes() == (plain / f).read_bytes(), f
    groups_equal_dmx_similarity(tmp_path, out, g, "s1")


def test_a_second_batch_is_refused_before_the_file_exists(tmp_path):
    g = tmp_path / "groups.tsv"
    _, r = _run(tmp_path, "two", "--groups", str(g), "--batch-mb", "1", check=False)
    assert r.returncode != 0 and "one resident batch" in r.stderr and not g.exists()
