"""Where the regions of the second-pass entries' device buffers lie (csrc/pdt_work_layout.h), without a GPU: tests/work_layout_main.cc
walks the five layouts -- ARGOS work, flywheel work, feed-forward work, repair work and the feed-forward result buffers with their shared
tail -- over a grid of small shapes under AddressSanitizer and UBSan: no two regions overlap, each is aligned for its elements, the last
ends at the total, and every offset equals the formula the entries wrote by hand before, rounded up to 16."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layouts_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "work_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "work_layout_main.cc")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # 2 x 3 x 4 shapes of the two bit-stream layouts, 2 x 2 x 2 of the feed-forward work, 2 of the repair, 3 x 4 of the two result buffers
    assert "work layout: ok, 82 layouts" in r.stdout and "Sanitizer" not in r.stderr, r.stdout + r.stderr
