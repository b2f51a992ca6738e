"""The MLP chain host code lives in ``sad_amd.mlp``; ``sad_amd.ops`` (and the package's lazy table) still spell every public
name, the switches stay in ``ops``, and the dispatch bookkeeping logs one entry per dispatch.  Needs no GPU and no built library."""
import os
import subprocess
import sys

import pytest

MOVED = ("PackedMLP", "PackedMLPBf16", "GroupedCall", "grouped_multi", "rowscan_multi", "cont_buffer", "workspace_status",
         "check_workspace", "choose_stage_assignment", "mlp_chain")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("LAUNCH_LOG", "RERUN_LOG", "AUTOTUNE", "GRID_MIN_POINTS", "MERGE_BF16", "SPLIT_POOL")


def test_moved_names_are_the_same_objects_everywhere():
    import sad_amd
    from sad_amd import mlp, ops
    for name in MOVED:
        assert getattr(ops, name) is getattr(mlp, name), name
    listed = [n for n in MOVED if n in sad_amd._LAZY]
    assert "PackedMLP" in listed and "mlp_chain" in listed
    for name in listed:
        assert getattr(sad_amd, name) is getattr(mlp, name), name
    assert ops.PackedMLP._CANDIDATES is mlp.PackedMLP._CANDIDATES and len(ops.PackedMLP._CANDIDATES) > 10
    from sad_amd.ops import choose_stage_assignment
    assert choose_stage_assignment is mlp.choose_stage_assignment
    assert choose_stage_assignment([2, 2], 1.0, {2: 1.0}, (2,)) == ([2, 2], 1.0)


def test_switches_live_in_ops_only():
    """``mlp`` reads ``ops.NAME`` at call time; a copy of a switch in ``mlp`` would go stale when a caller assigns ``ops.NAME``."""
    from sad_amd import mlp, ops
    for name in SWITCHES:
        assert hasattr(ops, name), name
        assert not hasattr(mlp, name), f"mlp.{name} shadows the switch in ops"


@pytest.mark.parametrize("first", ["mlp", "ops"])
def test_either_module_can_be_imported_first(first):
    other = "ops" if first == "mlp" else "mlp"
    code = (f"import sad_amd.{first} as a, sad_amd.{other} as b; "
            "from sad_amd import mlp, ops; assert ops.PackedMLP is mlp.PackedMLP and mlp.ops is ops")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_grouped_call_takes_8_9_and_10_elements():
    from sad_amd.ops import GroupedCall
    t = tuple(f"v{i}" for i in range(10))
    c8, c9, c10 = GroupedCall(*t[:8]), GroupedCall(*t[:9]), GroupedCall(*t)
    assert c8[:8] == t[:8] and c8.ws is None and c8.cont is None
    assert c9.ws == "v8" and c9.cont is None
    assert (c10.ws, c10.cont) == ("v8", "v9") and tuple(c10) == t
    assert GroupedCall._fields == ("mlp", "xyz", "feat_pm", "new_xyz", "idx", "out", "col_off", "cnt", "ws", "cont")
    assert GroupedCall(*c10) == c10
    with pytest.raises(TypeError):
        GroupedCall(*t[:7])


def test_dispatch_appends_one_rerun_entry_and_retries_once():
    from sad_amd import mlp, ops
    codes, alive = [], object()

    def enqueue():
        return codes.pop(0)
    assert ops.RERUN_LOG is None and ops.LAUNCH_LOG is None
    codes[:] = [0]
    mlp._dispatch("quiet", "fn", enqueue, alive, retry=lambda: pytest.fail("asked to retry a launch that succeeded"))
    assert codes == [] and ops.RERUN_LOG is None
    try:
        ops.RERUN_LOG = log = []
        asked = []
        codes[:] = [-2, 0]
        mlp._dispatch("a+b", "fn", enqueue, alive, retry=lambda: asked.append(1) or True)
        assert codes == [] and asked == [1]
        assert len(log) == 1 and log[0][0] == "a+b"
        assert log[0][1].__defaults__ == (alive,), "the entry does not hold the dispatch's tensors"
        codes[:] = [0]
        log[0][1]()
        assert codes == [] and len(log) == 1, "re-enqueueing must not log again"
    finally:
        ops.RERUN_LOG = None
