"""The band-mode key format on the host (no GPU): dmx_device.h's make_key_o / key_t_o / key_delta
in a stand-alone program (tests/origin_key_host.cpp) — the (t, delta) round trip, the same order
as make_key on every pair of cells that differs in another field, and the bound key with the
smallest delta code never above a real key of its cell."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_key_format_host_program(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "origin_key_host")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950",
                    "-I", os.path.join(ROOT, "nanopore-barcoding-orc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "origin_key_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
