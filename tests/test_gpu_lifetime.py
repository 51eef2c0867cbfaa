"""Resource lifetime of a prover: loading, proving once from a host witness (so the upload slot, its
pinned staging, copy streams and copy threads exist) and closing, six times over, must give the HBM
back.  Every device buffer, stream and event of the library is held by an owner of csrc/hip_raii.hpp;
a member that lost its owner would show here as one prover footprint per cycle.  With ZKP_INFLIGHT=2
the second pipeline shares the first one's base tables (shared_ptr<MsmBases>): they must go when the
last pipeline goes.

The HIP runtime itself keeps memory the first two times a process (or a new ZKP_INFLIGHT setting)
runs the prover's kernels on fresh streams: in a fresh process free HBM after close is 438 MB below
the start after cycle 1 and another 210 MB (ZKP_INFLIGHT=2: 260 MB) below after cycle 2, then
constant to the byte through cycle 6, before and after the owners were introduced alike.  Two
unmeasured cycles therefore come first; measured from there the footprint is 21 MB (35 to 38 MB) and the
drift over six cycles 0 bytes."""
import os

import pytest
import torch

import zkp_amd

pytestmark = pytest.mark.gpu
CYCLES = 6


def _free():
    torch.cuda.synchronize(0)
    return torch.cuda.mem_get_info(0)[0]


@pytest.mark.parametrize("inflight", [1, 2])
def test_prover_load_free_returns_memory(golden_dir, monkeypatch, inflight):
    monkeypatch.setenv("ZKP_INFLIGHT", str(inflight))
    zk = open(os.path.join(golden_dir, "circuit_small.zkey"), "rb").read()
    wt = open(os.path.join(golden_dir, "circuit_small.wtns"), "rb").read()
    for _ in range(2):  # the runtime's own one-time allocations (see above)
        prover = zkp_amd.Prover(zk, devices=[0])
        prover.prove(wt)
        prover.close()
    f0 = _free()
    footprint = None
    after = []
    for _ in range(CYCLES):
        prover = zkp_amd.Prover(zk, devices=[0])
        prover.prove(wt)
        if footprint is None:
            footprint = f0 - _free()
        prover.close()
        after.append(_free())
    drift = after[0] - after[-1]
    print("inflight %d: footprint %d B, free after each close %s, drift %d B" % (inflight, footprint, after, drift))
    assert footprint > 0
    # a cap, not a measurement: a prover-sized leak per cycle would be ~5 footprints
    assert drift <= footprint // 2
