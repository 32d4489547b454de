"""Every `file.rs:line` this repo cites must exist in the reference with those lines in range (tools/check_integration_refs.py);
for INTEGRATION.md -- the Rust shim that cannot be compiled here -- also every Rust identifier it quoted next to a citation.
The reference does not travel with the repository: the check runs against tests/golden/reference_index.json, which records
the line count of every source file of the reference and the quoted identifiers found in it
(tools/check_integration_refs.py --write-index, on a machine that has the tree)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX = os.path.join(ROOT, "tests", "golden", "reference_index.json")
DOCS = ["INTEGRATION.md", "DESIGN.md", "README.md", "include/dryv_recon.h", "oracle/dryv_oracle.c", "oracle/dryv_deblock.c",
        "dryv_amd/csrc/band_kernel.h", "dryv_amd/host/h264_islice.hpp", "dryv_amd/host/frame.hpp", "dryv_amd/host/frame_harness.cpp"]


def test_cited_reference_lines_exist():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_integration_refs.py"), "--index", INDEX]
                       + [os.path.join(ROOT, d) for d in DOCS], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "INTEGRATION.md: 3" in r.stdout   # (the shim's 36 citations were seen at all)
