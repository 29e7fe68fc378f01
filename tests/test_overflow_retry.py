"""The overflow retry of the main pipeline (dmx_exec_checked; csrc/dmx_api.cpp exec_checked,
grow_windows / grow_cands / grow_clusters).  The lists of a fresh context start at 8 n + 65536
records for n reads, so a few dozen long reads with an exact adapter copy every SPACING nt make
more windows than fit: a plain dmx_exec must report the window-overflow flag, dmx_exec_checked
must grow the lists and give the oracle's results, and a plain dmx_exec afterwards fits."""
import numpy as np
import pytest

import oracle
from dmx import lib, synth
from test_gpu_parity import _assert_same

pytestmark = pytest.mark.gpu

N_READS, COPIES, SPACING = 40, 3000, 256   # 120000 copies against 8 * 40 + 65536 window records
FLAG_WINDOWS = 4


@pytest.fixture(scope="module")
def planted():
    panel = synth.generate("c2x24", n=1, seed=3)["sp5"]
    rng = np.random.default_rng(8)
    codes = np.frombuffer(b"ACGT", dtype=np.uint8)
    ads = [np.frombuffer(a.encode(), dtype=np.uint8) for a in panel]
    seqs = []
    for _ in range(N_READS):
        s = codes[rng.integers(0, 4, size=COPIES * SPACING)]
        for k in range(COPIES):
            a = ads[int(rng.integers(len(ads)))]
            s[k * SPACING + 64:k * SPACING + 64 + len(a)] = a
        seqs.append(s.tobytes().decode())
    blob, offs, lens = oracle.pack_ascii(seqs)
    exp = oracle.run_batch(oracle.Panel(panel, oracle.FRONT), None, blob, offs, lens, mode=0,
                           threads=8)
    return panel, lib.pack(blob, offs, lens), exp


def test_window_overflow_is_grown_and_rerun(planted):
    panel, p, exp = planted
    with lib.Context(0) as c:
        c.set_panel(0, panel, lib.DMX_FRONT | lib.DMX_RC)
        c.set_mode(lib.MODE_SINGLE)
        c.load(p)
        c.exec()
        c.sync()
        st = c.stats()
        print("fresh context:", st["flags"], st["windows_raw"], st["filter_tasks"], st["tasks"])
        # the precondition: the window (or task) lists of a fresh context overflow
        assert st["flags"] & FLAG_WINDOWS, st
        c.exec_checked()
        _assert_same(c.fetch(), exp)
        c.exec()
        c.sync()
        st = c.stats()
        print("after the retry:", st["flags"], st["windows_raw"], st["filter_tasks"], st["tasks"])
        assert st["flags"] == 0, st
    assert (exp["bin1"] >= 0).all()
