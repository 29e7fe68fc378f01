"""One context through a sequence of shapes (ctx_sequence_cases.py): the buffers a context keeps
between calls, and the capacities read from them, must serve every later call as a fresh
context's would."""
import json
import os
import subprocess
import sys

import pytest

import ctx_sequence_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["two_round_512", "two_round_4096", "two_round_64", "views_300_of_64_reads",
         "linked_256_all_pairs", "chunked_3000_in_3", "run_100"]


def _assert_steps(out):
    assert list(out) == STEPS
    for name, (same_res, same_counts, matched) in out.items():
        assert same_res, f"{name}: results differ from a fresh context's"
        assert same_counts, f"{name}: counts differ from a fresh context's"
        assert matched > 0, f"{name}: nothing matched, the step checks nothing"


def test_one_context_equals_fresh_contexts():
    _assert_steps(sc.run_sequence())


def test_one_context_sequence_bounds_build():
    """The same under DMX_DEBUG_BOUNDS=1 (dmx/libdmx_bounds.so) in a child process: no access
    outside the extents the context reports for its buffers."""
    env = dict(os.environ, DMX_DEBUG_BOUNDS="1")
    env.pop("DMX_LIBDMX", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ctx_sequence_cases.py")],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["err"] == "", out["err"]
    _assert_steps(out["steps"])
