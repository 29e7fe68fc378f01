#!/usr/bin/env python3
"""Counters of the end-window kernels from rocprofv3 --pmc runs of
tools/bench_ends.py (one run per counter group; a group is never combined with a trace):

  rocprofv3 --pmc SQ_INSTS_VALU GRBM_GUI_ACTIVE SQ_INSTS_LDS --output-format csv -d A -o run -- \
      python3 tools/bench_ends.py --panels anchored,noninternal --repeats 1 --reads N
  rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT ... -d B ...

usage: ends_pmc_summary.py A B [OUT_JSON]

Per launch of ends_kernel (in launch order: per panel the warm-up exec, then the timed ones):
the VALU fraction = SQ_INSTS_VALU x 64 lanes over 256 CUs x 4 SIMDs x 32 lanes per clock at the
clock the launch ran at (GRBM_GUI_ACTIVE / 8 XCDs), as tools/kernel_table_from_pmc.py prices the
other kernels; LDS instructions per VALU instruction; the share of wave cycles spent waiting,
and waiting on LDS."""
import collections
import csv
import glob
import json
import os
import sys

VALU_LANES_PER_CLK = 256 * 4 * 32


def launches(d):
    paths = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"{d}: no counter_collection.csv")
    acc = collections.OrderedDict()
    for r in csv.DictReader(open(sorted(paths)[0])):
        if "ends_kernel" not in r["Kernel_Name"]:
            continue
        ent = acc.setdefault(int(r["Dispatch_Id"]), {
            "ms": (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6})
        ent[r["Counter_Name"]] = ent.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    return list(acc.values())


def main():
    a, b = launches(sys.argv[1]), launches(sys.argv[2])
    rows = []
    for x, y in zip(a, b):
        clk = x["GRBM_GUI_ACTIVE"] / 8.0 / (x["ms"] / 1e3)
        rows.append({
            "ms_under_counters": round(x["ms"], 3),
            "clock_ghz": round(clk / 1e9, 3),
            "valu_insts": x["SQ_INSTS_VALU"],
            "valu_frac_of_peak_at_clock":
                round(x["SQ_INSTS_VALU"] * 64 / (x["ms"] / 1e3) / (VALU_LANES_PER_CLK * clk), 4),
            "lds_insts_per_valu_inst": round(x["SQ_INSTS_LDS"] / max(1.0, x["SQ_INSTS_VALU"]), 4),
            "wait_frac": round(y["SQ_WAIT_ANY"] / max(1.0, y["SQ_WAVE_CYCLES"]), 4),
            "wait_lds_frac": round(y["SQ_WAIT_INST_LDS"] / max(1.0, y["SQ_WAVE_CYCLES"]), 4),
            "lds_conflict_cycles": y["SQ_LDS_BANK_CONFLICT"],
        })
    out = {"kernel": "ends_kernel<0>", "launches": rows,
           "source": "rocprofv3 --pmc, two runs of tools/bench_ends.py (counter groups apart)"}
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
