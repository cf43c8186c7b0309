"""debwt_amd/sharded.py over gloo on the collections that break one-GPU paths (tests/shard_cases.py): 2 and 3 ranks on the
box's one GPU, one launch per (world, key mode) -- the launcher and the torch import of every rank cost more than all builds
of a launch together -- in which every rank takes the cases one after the other through ONE context and workspace per k,
two builds each: a tiny collection with shards that own no key follows one with blocks above the LDS capacity and the other
way round.  The parent compares rank 0's gathered result of every case with the case's expected result."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import shard_cases as SC
from conftest import ROOT

MODES = ("exchange", "rescan", "scan")


WORKER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, %r)
    sys.path.insert(0, os.path.join(%r, "tests"))
    import numpy as np, torch
    from debwt_amd import api, sharded
    from debwt_amd import dist as D
    import shard_cases as SC
    rank, local_rank, world = D.init(backend="gloo")
    torch.cuda.set_device(0)                              # every rank on the one GPU of the test box
    out, mode = sys.argv[1], sys.argv[2]
    ctx, res = {}, {}
    for i, name in enumerate(SC.sharded_launch_cases(world)):
        c = SC.CASES[name]
        if c.k not in ctx:
            d = api.DeBWT(k=c.k, device=0)
            ctx[c.k] = (d, sharded.Workspace(d, torch.device("cuda", 0), mode=mode))
        d, ws = ctx[c.k]
        d.load_records(c.records())
        for it in range(2):                               # a context is reusable in sharded mode, whatever it built before
            info = sharded.build_sharded(d, ws)
        assert info["keys"] == mode, info
        got = sharded.gather_bwt(d, c.n, ws)
        if rank == 0:
            res["w%%d" %% i], res["h%%d" %% i], res["d%%d" %% i] = got[0], got[1], np.array([got[2]], dtype=np.uint64)
    if rank == 0:
        np.savez(out, **res)
    D.finalize()
    for d, ws in ctx.values():
        d.close()
""") % (ROOT, ROOT)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("world", [2, 3])
# (world <= 4: see tests/test_sharded.py; 8 shards of these collections: tests/test_multi_shard_edges_gpu.py)
def test_sharded_builds_of_the_edge_collections(tmp_path, oracle, world, mode):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    out = str(tmp_path / "res.npz")
    port = str(29700 + 10 * world + MODES.index(mode))                   # (tests/test_sharded.py: 29540..29620)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", port, str(script), out, mode]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    z = np.load(out)
    names = SC.sharded_launch_cases(world)
    assert len(z.files) == 3 * len(names)
    for i, name in enumerate(names):
        diff = SC.check_result(name, oracle, z[f"w{i}"], z[f"h{i}"], int(z[f"d{i}"][0]))
        assert diff is None, (world, mode, i, name, diff)


def test_every_launch_has_empty_shards_small_shards_and_a_large_block_behind_a_block_base():
    """What the launches reach, from the plan alone (sharded.plan_splitters cuts as the C host does:
    tests/test_shard_cases_ref.py)."""
    for world in (2, 3):
        names = SC.sharded_launch_cases(world)
        plans = [SC.plan_case(nm, world) for nm in names]
        assert any(min(p.keys) == 0 for p in plans)                                   # a shard without keys
        assert any(p.slices[0] == (0, 0) for p in plans)                              # a slice without positions
        assert any(1 <= min(p.keys) <= 15 for p in plans)                             # shards of a handful of keys
        assert SC.plan_case("blocks_first_middle_last", world).blocks[world - 1].max() > 2048
        assert sum(1 for nm in names if SC.CASES[nm].edges) == {2: 8, 3: 4}[world]     # every kind of slice edge, k = 12 and 32
        assert {SC.CASES[nm].k for nm in names} == {12, 32}
