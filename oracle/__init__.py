"""CPU restatement of the reference's reconstruction path — TEST INFRASTRUCTURE ONLY.

Only tests/, the checks of tools/ (tools/inter_rate.py compares its pictures with inter_model),
__graft_entry__.smoke() and bench.py's cpu_baseline leg may import this package; nothing under
dryv_amd/ does, and nothing here imports from tests/. PARITY UNPINNED (see dryv_oracle.c header and DESIGN.md).
"""
from .oracle import build, load, reconstruct, decode_mb, residual4x4, residual8x8, get_qpc, deblock  # noqa: F401
