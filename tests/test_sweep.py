"""GPU parity of the random-panel slice (sweep_cases.py) against the oracle.

Every fixed case runs in the default configuration, and in every configuration that changes the
path its panel takes: the per-part screen instead of the flat scan, 64-position parts, one
orientation, the full filter pass instead of the piece screen, the window scan without the index
screen or with the unpacked one, near pieces scanned for every adapter, no prefix verification,
no filter, the ring resolve, a chunked run, a permuted batch.  All 40 result bytes of every read
must equal the oracle's, and the path the variant claims must have run (filter tasks).  A failing
(case, variant) replays with

    python tools/parity_sweep.py --case <case id> [--env NAME=VALUE ...]

test_sweep_host.py (CPU) holds the census that keeps the cases on these paths."""
import functools

import numpy as np
import pytest

import sweep_cases as sw
from dmx import lib

pytestmark = pytest.mark.gpu

STEPS = ("step1", "step2", "step4")
# variant: (environment, the strata it applies to); "n/3" becomes a third of the batch
VARIANTS = {
    "default": ({}, sw.STRATA),
    "no_flat": ({"DMX_NO_FLAT": "1"}, STEPS + ("near", "pair2")),
    "no_flat_part64": ({"DMX_NO_FLAT": "1", "DMX_PIECE_PART": "64"}, STEPS),
    "one_orient": ({}, STEPS),
    "no_pieces": ({"DMX_NO_PIECES": "1"}, STEPS + ("near",)),
    "no_screen": ({"DMX_NO_SCREEN": "1"}, ("filter", "step2", "near", "pair2")),
    "screen_v1": ({"DMX_SCREEN_V1": "1"}, ("filter", "step2", "near")),
    "near_all": ({"DMX_NEAR_ALL": "1"}, ("near",)),
    "no_verify": ({"DMX_NO_VERIFY": "1"}, ("filter", "step2")),
    "no_filter": ({"DMX_NO_FILTER": "1"}, ("filter", "step2")),
    "ring": ({"DMX_RESOLVE": "ring"}, ("plain", "step2", "pair2")),
    "chunked": ({"DMX_RUN_CHUNK": "n/3"}, ("pair2", "step2:first")),
    "permuted": ({}, tuple(s + ":first" for s in STEPS)),
}


def _params():
    out, seen = [], set()
    for cid in sw.fixed_ids():
        st = cid.rsplit("-", 1)[0]
        tags = (st,) if st in seen else (st, st + ":first")
        seen.add(st)
        out += [(cid, v) for v, (_, strata) in VARIANTS.items() if set(tags) & set(strata)]
    return out


@functools.lru_cache(maxsize=None)
def _case(cid):
    case = sw.build_case(cid)
    return case, sw.pack(case)


@functools.lru_cache(maxsize=None)
def _expected(cid, use_rc):
    return sw.expected(_case(cid)[0], use_rc)


def _run(c, case, p, use_rc, chunked):
    sw.set_panels(c, case, use_rc)
    got = c.run(p)
    if chunked:   # a chunked run keeps no whole result set on the device (test_chunked_run.py)
        with pytest.raises(lib.DmxError):
            c.fetch()
    return got, c.stats()["filter_tasks"], int(c.debug_fetch(lib.DBG_FLAGS, 0)[0])


@pytest.mark.parametrize("cid,variant", _params(), ids=lambda x: x)
def test_sweep_case(cid, variant, ctx, monkeypatch):
    case, p = _case(cid)
    use_rc = case["rc"] and variant != "one_orient"
    exp = _expected(cid, use_rc)
    screened = [x["step"] > 0 and case["kind"] != "linked" for x in sw.classify(case, use_rc)]
    perm = None
    if variant == "permuted":   # as test_pieces._run: the same packed nt, reads in another order
        perm = np.random.default_rng(1).permutation(p.n_reads)
        p = lib.Packed(p.seq2b, p.nmask, p.offsets[perm].copy(), p.lengths[perm].copy())
    env = {k: str(p.n_reads // 3) if v == "n/3" else v for k, v in VARIANTS[variant][0].items()}
    if variant == "default":
        got, tasks, flags = _run(ctx, case, p, use_rc, False)
    else:   # the switches are read in dmx_open, dmx_set_panel and at the run
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with lib.Context(0) as c:
            got, tasks, flags = _run(c, case, p, use_rc, variant == "chunked")
    if perm is not None:
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        got = got[inv]
    replay = f"python tools/parity_sweep.py --case {cid}" + \
        "".join(f" --env {k}={v}" for k, v in env.items())
    bad = sw.differing(got, exp)
    assert len(bad) == 0, f"{cid} [{variant}]: {len(bad)} reads differ, first {bad[:10]}; {replay}"
    assert flags & (16 | 4) == 0, f"{cid} [{variant}]: pipeline flags {flags}; {replay}"
    for r, on in enumerate(screened):
        if variant == "no_pieces" or case["stratum"] in ("plain", "filter"):
            assert tasks[r] == 0, f"{cid} [{variant}]: filter tasks {tasks} in round {r}; {replay}"
        elif on and variant != "no_filter":
            assert tasks[r] > 0, f"{cid} [{variant}]: no filter tasks in round {r}; {replay}"
