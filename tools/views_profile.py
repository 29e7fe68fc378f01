"""DMX_PROFILE_IO of `dmx-demux-loop --reorient` with and without `--device-views` (DESIGN.md
§3.17): what keeping pychopper's PASS segments on the GPU saves over packing and uploading them
as a second batch.

Generates `--reads` raw reads of workload c2 as a plain FASTQ (tools/e2e_bench.py's writer),
then runs the loop `--runs` times each way, alternating, on one device, and writes the
per-phase table (seconds, per run and mean) as Markdown:

    python tools/views_profile.py --reads 1000000 --runs 4 --out profiles/views_profile_1M.md
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import e2e_bench as e2e  # noqa: E402  (FASTQ writer; puts the package on sys.path)
from dmx import synth  # noqa: E402

LOOP = os.path.join(e2e.PKG, "bin", "dmx-demux-loop")
PHASES = ("wall", "read_wait", "gpu", "reo", "reo_qual", "reo_tune", "reo_chop", "reo_rows",
          "views", "pack", "plan_write", "drain")


def one_run(raw: str, wd: str, tag: str, threads: int, flags: list) -> dict:
    out = os.path.join(wd, tag)
    shutil.rmtree(out, ignore_errors=True)
    t = time.perf_counter()
    p = subprocess.run([LOOP, raw, "--reorient", "--device", "0", "-j", str(threads),
                        "--pychopper-dir", os.path.join(out, "pychopped"),
                        "--outdir", os.path.join(out, "demuxed")] + flags,
                       env=dict(os.environ, DMX_PROFILE_IO="1"), stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True, check=True)
    wall = time.perf_counter() - t
    line = [ln for ln in p.stderr.splitlines() if ln.startswith("io profile (s):")][-1]
    prof = {k: float(v) for k, v in re.findall(r"(\w+) ([0-9.]+)[,;]", line.split("phases")[0])}
    prof["wall"] = wall
    shutil.rmtree(out, ignore_errors=True)
    return prof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    wd = tempfile.mkdtemp(prefix="dmx_views_profile_")
    raw = os.path.join(wd, "raw.fastq")
    e2e.write_fastq(raw, synth.generate("c2", n=a.reads, seed=77), seed=5)
    arms = (("packed", []), ("device_views", ["--device-views"]))
    runs = {name: [] for name, _ in arms}
    for i in range(a.runs):
        for name, flags in arms:
            runs[name].append(one_run(raw, wd, name, a.threads, flags))
            print(f"run {i + 1} {name}: " + ", ".join(f"{k} {runs[name][-1].get(k, 0.0):.3f}"
                                                      for k in PHASES), flush=True)
    shutil.rmtree(wd, ignore_errors=True)
    lines = [f"# `dmx-demux-loop --reorient` with and without `--device-views`: {a.reads:,} raw "
             f"reads (c2), plain FASTQ, {a.threads} host threads, one device",
             "",
             f"Seconds per phase (`DMX_PROFILE_IO`), {a.runs} runs each, alternating; `wall` is "
             "the whole process, `gpu` holds `reo` (its parts: `reo_*`), `pack` and the "
             "demultiplexer (`views`: exec, fetch and the list, with the flag).",
             "",
             "| phase | " + " | ".join(f"{name} {i + 1}" for name, _ in arms
                                       for i in range(a.runs)) + " | packed mean | "
             "device_views mean | difference |",
             "|---|" + "---|" * (2 * a.runs + 3)]
    for k in PHASES:
        vals = {name: [r.get(k, 0.0) for r in runs[name]] for name, _ in arms}
        mean = {name: sum(v) / len(v) for name, v in vals.items()}
        lines.append(f"| {k} | " + " | ".join(f"{x:.3f}" for name, _ in arms for x in vals[name])
                     + f" | {mean['packed']:.3f} | {mean['device_views']:.3f} | "
                     f"{mean['device_views'] - mean['packed']:+.3f} |")
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
