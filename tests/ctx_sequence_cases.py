"""One context through a sequence of shapes (tests/test_ctx_sequence.py).

The host context grows its device buffers on demand and keeps them between calls; every step
below changes which of them are too small: more reads, fewer reads, more views than reads, a
linked batch whose item list outgrows the winner slots, a chunked dmx_run (two input sets,
swapped per chunk) and a plain dmx_run after it.  After every step the results and counts on the
one long-lived context must equal, byte for byte, the same call on a fresh context.

Imported by the GPU test (release library, in-process) and run as a script under
DMX_DEBUG_BOUNDS=1 (dmx/libdmx_bounds.so, in a child process), where every gather and slot access
is checked against the extents the context reports for its buffers.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "nanopore-barcoding-orc_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle  # noqa: E402  (pack_ascii only)
from dmx import lib, synth  # noqa: E402

SEED = 77
CHUNK = 1000   # DMX_RUN_CHUNK of the chunked step: 3000 reads make 3 chunks


def _short(d, keep=100):
    """The generator's reads cut to about 200 nt: the first and last `keep` nt of each (both
    adapters stay), as strings."""
    out = []
    for o, n in zip(d["offsets"], d["lengths"]):
        s = bytes(d["blob"][int(o):int(o) + int(n)]).decode()
        out.append(s if len(s) <= 2 * keep else s[:keep] + s[-keep:])
    return out


def _data():
    d = synth.generate("c2x24", n=4096, seed=SEED)
    return d, _short(d)


def _pack(seqs):
    blob, offs, lens = oracle.pack_ascii(seqs)
    return lib.pack(blob, offs, lens)


def _two_round(ctx, d):
    ctx.clear_views()
    ctx.set_panel(0, d["sp5"], lib.DMX_FRONT | lib.DMX_RC)
    ctx.set_panel(1, d["sp27"], lib.DMX_BACK | lib.DMX_RC)
    ctx.set_mode(lib.MODE_TWO_ROUND)


def _out(res, ctx):
    return res.tobytes(), ctx.counts().tolist()


def steps():
    """[(name, fn(ctx) -> (result bytes, counts))]: each sets its own panels and mode, so it runs
    the same on a fresh context."""
    d, seqs = _data()
    rng = np.random.default_rng(SEED)

    def plain(n):
        def fn(ctx):
            _two_round(ctx, d)
            return _out(ctx.run(_pack(seqs[:n])), ctx)
        return fn

    n_views = 300
    v_read = rng.integers(0, 64, size=n_views)
    v_len = np.array([len(seqs[r]) for r in v_read])
    v_start = (rng.random(n_views) * v_len * 0.3).astype(np.int32)
    v_stop = (v_len - rng.random(n_views) * v_len * 0.3).astype(np.int32)
    v_strand = rng.integers(0, 2, size=n_views)

    def views(ctx):
        _two_round(ctx, d)
        ctx.load(_pack(seqs[:64]))
        ctx.set_views(v_read, v_start, v_stop, v_strand)
        ctx.exec_checked()
        out = _out(ctx.fetch(), ctx)
        ctx.clear_views()
        return out

    # linked: every read carries every pair, so round 1 has reads x pairs items
    dna = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    pairs = [(dna(22), dna(24)) for _ in range(3)]
    lseqs = []
    for _ in range(256):
        s = ""
        for f, r in pairs:
            s += dna(int(rng.integers(0, 10))) + f + dna(int(rng.integers(20, 40))) + r
        lseqs.append(s)

    def linked(ctx):
        ctx.clear_views()
        ctx.set_panel(0, [p[0] for p in pairs], lib.DMX_FRONT)
        ctx.set_panel(1, [p[1] for p in pairs], lib.DMX_BACK)
        ctx.set_mode(lib.MODE_LINKED)
        return _out(ctx.run(_pack(lseqs)), ctx)

    def chunked(ctx):
        _two_round(ctx, d)
        old = os.environ.get("DMX_RUN_CHUNK")
        os.environ["DMX_RUN_CHUNK"] = str(CHUNK)
        try:
            out = _out(ctx.run(_pack(seqs[:3000])), ctx)
            try:   # a chunked run's results went to the caller: dmx_fetch is refused after it
                ctx.fetch()
            except lib.DmxError:
                return out
            raise AssertionError("the run of 3000 reads was not chunked")
        finally:
            if old is None:
                del os.environ["DMX_RUN_CHUNK"]
            else:
                os.environ["DMX_RUN_CHUNK"] = old

    return [("two_round_512", plain(512)), ("two_round_4096", plain(4096)),
            ("two_round_64", plain(64)), ("views_300_of_64_reads", views),
            ("linked_256_all_pairs", linked), ("chunked_3000_in_3", chunked),
            ("run_100", plain(100))]


def run_sequence():
    """Every step on one context and on a fresh one: {step: [result bytes equal, counts equal,
    reads matched on the fresh context]}."""
    out = {}
    with lib.Context(0) as ctx:
        for name, fn in steps():
            got, got_counts = fn(ctx)
            with lib.Context(0) as fresh:
                exp, exp_counts = fn(fresh)
            res = np.frombuffer(exp, dtype=lib.RESULT_DTYPE)
            out[name] = [got == exp, got_counts == exp_counts, int((res["bin1"] >= 0).sum())]
    return out


def main():
    assert lib.BOUNDS and lib.LIB_PATH.endswith("libdmx_bounds.so"), lib.LIB_PATH
    try:
        print(json.dumps({"steps": run_sequence(), "err": ""}), flush=True)
    except lib.DmxError as e:
        print(json.dumps({"steps": {}, "err": str(e)}), flush=True)


if __name__ == "__main__":
    main()
