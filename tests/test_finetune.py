"""dmx.sorter.finetune through a Context: the lock-step schedule on
dmx_pairdist, dmx_rowdist, dmx_groupalign_strands and dmx_rowpairdist against the same call with
ctx=None, which tests/test_finetune_host.py pins to the literal model of the reference; on lists,
on resident operands of a demultiplexer run, with the pair lists cut into small launches, as
rest_reads' hook and behind `dmx-similarity --finetune`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import finetune_cases as fc
import operands_cases as oc
import views_cases as vc
from dmx import lib, sorter
from test_finetune_host import as_lists, rest_expected

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nanopore-barcoding-orc_amd", "bin", "dmx-similarity")


@functools.lru_cache(maxsize=None)
def host_answer(cycles=10):
    reads, groups, cons = fc.all_cases()
    return sorter.finetune(None, reads, groups, cons, max_cycles=cycles)


def same(got, exp):
    assert as_lists(got[0]) == as_lists(exp[0])
    assert list(got[1]) == list(exp[1])


@pytest.mark.parametrize("cycles", [10, 2])
def test_all_cases_in_one_call(ctx, cycles):
    reads, groups, cons = fc.all_cases()
    same(sorter.finetune(ctx, reads, groups, cons, max_cycles=cycles), host_answer(cycles))
    assert ctx._resident is reads               # the batch of an unchanged list stays resident
    gen = ctx._load_gen
    same(sorter.finetune(ctx, reads, groups[1:2], cons[1:2]),
         sorter.finetune(None, reads, groups[1:2], cons[1:2]))
    assert ctx._load_gen == gen                 # and the next call runs on it as it lies


def test_small_launches(ctx, monkeypatch):
    reads, groups, cons = fc.all_cases()
    monkeypatch.setenv("DMX_PD_CHUNK", "37")
    got = sorter.finetune(ctx, reads, groups, cons)
    monkeypatch.delenv("DMX_PD_CHUNK")
    same(got, host_answer())


@pytest.fixture(scope="module")
def demuxed():
    """The cases' reads as operands of a demultiplexer run: every read between one SP5 and one
    SP27 adapter and random flanks, a third of the records stored reverse-complemented, run
    through the benchmark's two rounds; the well's operands are the reads again."""
    reads, _, _ = fc.all_cases()
    rng = np.random.default_rng(838)
    sp5, sp27 = vc.bench_panels()
    raw = []
    for r in reads:
        s = (oc.rand_seq(rng, rng.integers(0, 25)) + sp5[2] + r + sp27[1] +
             oc.rand_seq(rng, rng.integers(0, 25)))
        raw.append(oc.revcomp(s) if rng.random() < 0.33 else s)
    with lib.Context(0) as c:
        c.set_panel(0, sp5, lib.DMX_FRONT | lib.DMX_RC, 0.1, 3)
        c.set_panel(1, sp27, lib.DMX_BACK | lib.DMX_RC, 0.1, 3)
        c.set_mode(lib.MODE_TWO_ROUND)
        c.load(oc.pack(raw))
        c.exec_checked()
        first = c.result_operands(None, 50)
        well = (2 + 1) * (len(sp27) + 1) + (1 + 1)
        yield c, sorter.Operands(c, raw).bin(first, well)


def test_operands_of_a_demultiplexer_run(demuxed):
    c, ops = demuxed
    reads, groups, cons = fc.all_cases()
    assert len(ops) == len(reads) and set(ops.strand.tolist()) == {0, 1}
    seqs = [ops[k] for k in range(len(ops))]
    # the trimmed reads are the cases' reads (a chance base of a flank aside)
    assert sum(s.decode() == r for s, r in zip(seqs, reads)) >= 0.9 * len(reads)
    exp = (host_answer() if [s.decode() for s in seqs] == reads
           else sorter.finetune(None, seqs, groups, cons))
    same(sorter.finetune(c, ops, groups, cons), exp)


def test_outcomes_and_the_resident_batch_survive(demuxed):
    c, ops = demuxed
    _, groups, cons = fc.all_cases()
    ops.activate()
    g = groups[1]
    q, t = np.repeat(g[:6], 6), np.tile(g[6:12], 6)
    ln = ops.lengths
    cap = np.array([sorter.identity_cap(int(max(ln[a], ln[b])), 0.8) for a, b in zip(q, t)])
    half = np.array([sorter.identity_cap(int(max(ln[a], ln[b])), 0.5) for a, b in zip(q, t)])
    best, n_hits = c.pairhits(q, t, cap, half)
    before = c.pairhits_fetch()
    assert n_hits >= 6
    gen, table = c._load_gen, c.operands()
    sorter.finetune(c, ops, groups, cons)
    assert c._load_gen == gen and c._resident is ops
    for a, b in zip(c.operands(), table):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(c.pairhits_fetch(), before):
        np.testing.assert_array_equal(a, b)


def test_rest_reads_with_finetune_as_its_hook(ctx):
    reads, indexes, groups, _, _ = fc.rest_bin()
    exp, _, cons = rest_expected()
    assert sorter.species_consensuses(ctx, reads, groups) == cons
    got = sorter.rest_reads(ctx, reads, indexes, groups, cons,
                            finetune=functools.partial(sorter.finetune, ctx, reads))
    same(got, exp)
    assert len(got[0]) == 2


@functools.lru_cache(maxsize=None)
def cli_bin():
    """fc.rest_bin()'s reads as a bin file's: at -ssg 86 both species start in one species
    group.  What sort_species makes of it on the host twins with and without finetune."""
    reads = fc.rest_bin()[0]
    genes = sorter.gene_groups(None, reads)
    species = sorter.species_groups(None, reads, genes, 86.0)
    assert [len(sp) for sp in species] == [1]
    hook = functools.partial(sorter.finetune, None, reads)
    return (reads, sorter.sort_species(None, reads, genes, species, finetune=hook),
            sorter.sort_species(None, reads, genes, species, finetune=None))


def _run_cli(tmp_path, reads, *flags):
    src = tmp_path / "bin.fastq"
    src.write_text("".join(f"@read{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)))
    out = tmp_path / "assigned.txt"
    r = subprocess.run([sys.executable, CLI, "-i", str(src), "--groups", str(tmp_path / "g.txt"),
                        "--species-groups", str(tmp_path / "s.txt"), "-ssg", "86",
                        "--assigned", str(out), *flags], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text(), (tmp_path / "assigned.txt.fasta").read_text()


@pytest.mark.parametrize("flag", ["--finetune", None])
def test_cli_writes_what_the_library_gives(tmp_path, flag):
    """With --finetune the files of the ctx=None route with the hook; without it the files of
    sort_species(..., finetune=None), the code path before the flag existed."""
    reads, with_hook, without = cli_bin()
    exp = tmp_path / "exp.txt"
    sorter.write_assigned(str(exp), with_hook if flag else without, 85.0, 96.0, 8.0)
    text, fasta = _run_cli(tmp_path, reads, *([flag] if flag else []))
    assert text == exp.read_text()
    assert fasta == (tmp_path / "exp.txt.fasta").read_text()
    # the blended group without the flag, the two species with it
    assert len(text.splitlines()) == (3 if flag else 2)
    assert [len(g) for _, g, _ in (with_hook, without)[flag is None]] == [2 if flag else 1]


def test_finetune_alone_is_refused(tmp_path):
    src = tmp_path / "bin.fastq"
    src.write_text("@r\nACGT\n+\nIIII\n")
    r = subprocess.run([sys.executable, CLI, "-i", str(src), "--groups", str(tmp_path / "g.txt"),
                        "--finetune"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--finetune needs --assigned" in r.stderr
    assert not (tmp_path / "g.txt").exists()
