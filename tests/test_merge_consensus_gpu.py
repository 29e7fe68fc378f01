"""sorter.compare_consensuses / comp_consensus_groups on the GPU (dmx_rowhits)
against the same calls on the host twins, and dmx-similarity --merged-groups against the library
call."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rowpair_cases as rp
from dmx import sorter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nanopore-barcoding-orc_amd", "bin", "dmx-similarity")


def as_lists(groups):
    return [[int(x) for x in g] for g in groups]


def test_compare_consensuses_equals_the_host(ctx):
    reads, groups, _ = rp.split_bin()
    cons = sorter.make_consensus(None, reads, groups, n_threads=8)
    exp = sorter.compare_consensuses(None, cons, n_threads=8)
    assert len(exp) == 3
    assert sorter.compare_consensuses(ctx, cons) == exp
    # a lower threshold and a wider length rule: more lines, the same on both sides
    assert sorter.compare_consensuses(ctx, cons, 30.0, 0.40) == \
        sorter.compare_consensuses(None, cons, 30.0, 0.40, n_threads=8)


def test_comp_consensus_groups_equals_the_host(ctx):
    reads, groups, fam = rp.split_bin()
    exp = sorter.comp_consensus_groups(None, reads, groups, n_threads=8)
    got = sorter.comp_consensus_groups(ctx, reads, groups)
    assert as_lists(got) == as_lists(exp) and len(got) == 3
    g2, c2 = sorter.compare_consensus(ctx, reads, groups,
                                      sorter.make_consensus(None, reads, groups, n_threads=8), 90.0)
    e2, ec2 = sorter.compare_consensus(None, reads, groups,
                                       sorter.make_consensus(None, reads, groups, n_threads=8),
                                       90.0, n_threads=8)
    assert as_lists(g2) == as_lists(e2) and c2 == ec2


def test_cli_writes_the_merged_groups(tmp_path):
    reads, _, _ = rp.split_bin()
    src = tmp_path / "bin.fastq"
    src.write_text("".join(f"@read{i}\n{r.decode()}\n+\n{'I' * len(r)}\n"
                           for i, r in enumerate(reads)))
    grp, out = tmp_path / "groups.txt", tmp_path / "merged.txt"
    r = subprocess.run([sys.executable, CLI, "-i", str(src), "--groups", str(grp),
                        "--merged-groups", str(out), "-min", "0"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    groups = [np.array(line.split(), dtype=np.int64) for line in grp.read_text().splitlines()]
    exp = sorter.comp_consensus_groups(None, reads, groups, n_threads=8)
    assert out.read_text() == "".join(" ".join(str(int(x)) for x in g) + "\n" for g in exp)
    assert len(exp) >= 1

