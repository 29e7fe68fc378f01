"""The three row forms in sequence on one context (csrc/dmx_pd_rows.h PdRows):
dmx_rowassign, dmx_rowdist, dmx_rowpairdist and dmx_rowhits share one type for a call's rows on
the device, and nothing of it but buffer capacity may pass from one call into the next.  Nine
calls on row sets of their own (rowset_cases.py), each compared with its host twin; then the same
sequence in a child process on the bounds-checked library, where the forward pass is checked
against the columns actually written."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rowset_cases as rs
from dmx import lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nanopore-barcoding-orc_amd")


@pytest.fixture(scope="module")
def seq():
    c = rs.case()
    exp = [rs.expected(c, k) for k in range(len(c["steps"]))]
    rs.check_coverage(c, exp)
    return c, exp


def same(got, exp, name):
    assert len(got) == len(exp), name
    for j, (g, e) in enumerate(zip(got, exp)):
        np.testing.assert_array_equal(np.asarray(g), np.asarray(e), err_msg=f"step {name}, output {j}")


def test_sequence_on_one_context(ctx, seq, monkeypatch):
    c, exp = seq
    monkeypatch.setenv("DMX_PD_CHUNK", rs.CHUNK)
    bad = []   # every step runs: a failure names all the steps that differ, not the first
    for k, (name, _, _) in enumerate(c["steps"]):
        try:
            same(rs.run(ctx, c, k), exp[k], name)
        except AssertionError as e:
            bad.append(f"{name}: {str(e).strip().splitlines()[-1]}")
    assert not bad, "\n".join(bad)


CHILD = """import sys, json
sys.path[:0] = [{tests!r}, {pkg!r}, {oracle!r}]
import rowset_cases as rs
from dmx import lib
c = rs.case()
out = {{'lib': lib.LIB_PATH, 'steps': []}}
with lib.Context(0) as ctx:
    for k, (name, _, _) in enumerate(c['steps']):
        try:
            out['steps'].append([x.tolist() for x in rs.run(ctx, c, k)])
        except lib.DmxError as e:
            out['failed'] = name + ': ' + str(e)
            break
print(json.dumps(out))
"""


def test_sequence_on_the_bounds_build(seq, tmp_path):
    c, exp = seq
    script = tmp_path / "run.py"
    script.write_text(CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=PKG,
                                   oracle=os.path.join(ROOT, "oracle")))
    env = dict(os.environ, DMX_DEBUG_BOUNDS="1", DMX_PD_CHUNK=rs.CHUNK)
    env.pop("DMX_LIBDMX", None)
    res = subprocess.run([sys.executable, str(script)], capture_output=True, text=True,
                         timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["lib"].endswith("libdmx_bounds.so")
    assert "failed" not in out, "step " + out.get("failed", "")
    for k, (name, _, _) in enumerate(c["steps"]):
        same(out["steps"][k], exp[k], name)
