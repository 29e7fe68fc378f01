"""dmx.sorter.assign_best, rest_reads and the --assigned output of dmx-similarity through a
Context (dmx_rowassign's kernels under the loop) against the same calls with
ctx=None, which test_assign_best.py pins to the literal restatement of the reference."""
import os
import subprocess
import sys

import pytest

import test_assign_best as tb
from dmx import sorter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nanopore-barcoding-orc_amd", "bin", "dmx-similarity")


def test_assign_best_on_the_gpu(ctx):
    reads, unassigned, cons = tb.ta.make_bin()
    for similar in (0.95, 0.90, 0.85):
        assert sorter.assign_best(ctx, reads, unassigned, cons, similar) == \
            sorter.assign_best(None, reads, unassigned, cons, similar)
        assert ctx.rowassign_ms() > 0
    assert ctx._resident is reads               # the batch of an unchanged list stays resident
    assert sorter.assign_best(ctx, reads, unassigned, cons, 0.93, chunk=50, max_chunks=2) == \
        sorter.assign_best(None, reads, unassigned, cons, 0.93, chunk=50, max_chunks=2)
    assert sorter.assign_best(ctx, reads, [], cons, 0.93) == ([], [])


def test_rest_reads_on_the_gpu(ctx):
    reads, indexes, groups, cons, (g, c, _) = tb.rest_case()
    assert sorter.species_consensuses(ctx, reads, groups) == cons
    got_g, got_c = sorter.rest_reads(ctx, reads, indexes, groups, cons)
    assert [x.tolist() for x in got_g] == g
    assert got_c == c


def test_cli_assigned_writes_what_the_library_gives(tmp_path):
    reads, _, _ = tb.species_bin(seed=96, per=39)
    assert 115 <= len(reads) <= 125
    src = tmp_path / "bin.fastq"
    src.write_text("".join(f"@read{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)))
    genes = sorter.gene_groups(None, reads)
    species = sorter.species_groups(None, reads, genes, 97.0)
    assert len(genes) == 3 and all(len(sp) >= 1 for sp in species)
    done = sorter.sort_species(None, reads, genes, species)
    assert sum(len(x) for _, gs, _ in done for x in gs) > sum(len(m) for sp in species for m in sp)
    exp = tmp_path / "exp.txt"
    sorter.write_assigned(str(exp), done, 85.0, 96.0, 8.0)
    out = tmp_path / "assigned.txt"
    r = subprocess.run([sys.executable, CLI, "-i", str(src), "--groups", str(tmp_path / "g.txt"),
                        "--species-groups", str(tmp_path / "s.txt"), "-ssg", "97",
                        "--assigned", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_text() == exp.read_text()
    assert (tmp_path / "assigned.txt.fasta").read_text() == (tmp_path / "exp.txt.fasta").read_text()
    assert len(out.read_text().splitlines()) >= 4 and "final species groups" in r.stderr
