"""The host side of the ingest without a GPU: tests/ingest_host_main.cc -- a stand-alone program over csrc/pdt_ingest.h (layout
table, cpulist parser, read loop, page-cache probe, and the ring of slots with a memcpy copier: clean runs and wind-down) --
built once with the address and undefined-behaviour sanitizers and once with the thread sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_ingest_host(sanitizer, tmp_path):
    exe = str(tmp_path / "ingest_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "ingest_host_main.cc")], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ingest host: ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout + r.stderr
