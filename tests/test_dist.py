"""world_size-2 tests of the multi-process path (gloo, 127.0.0.1).

CPU: the distributed helpers bench.py and the sharded BA rely on (max over ranks, sequence sharding, the
all-reduce callback driven through its C function pointer).
GPU: the landmark-sharded local BA (fb_local_ba_sharded), two ranks sharing the one GPU of the box, against the ORACLE
(8 key frames, and 20 key frames x 8000 + 2000 points = BASELINE configs[4]'s BA; stop flag raised on one rank only);
the RCCL transport on a 1-rank communicator, and -- only on a box with >= 2 GPUs -- on a real 2-rank communicator
(fresh child processes, one GPU each).  Multi-rank RCCL has never executed where these tests have run so far."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_world2(mode, timeout=240):
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_worker.py"), mode], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode())
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, o)
    return outs


def test_distributed_helpers_world2_gloo():
    outs = _run_world2("helpers")
    assert all("helpers ok" in o for o in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ba", "ba_config5"])
def test_sharded_local_ba_world2_vs_oracle(mode):
    """Two ranks (landmark partition) against the CPU oracle of the unsharded problem; "ba_config5" has the shape of BASELINE
    config 5's BA (20 key frames x 8000 + 2000 points)."""
    outs = _run_world2(mode)
    assert all("flags_equal=True" in o and "identical_across_ranks=True" in o for o in outs)


@pytest.mark.gpu
def test_sharded_local_ba_stop_flag_on_one_rank():
    outs = _run_world2("ba_stop", timeout=120)
    assert all("identical_across_ranks=True" in o for o in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ba_rccl", "ba_rccl_stop"])
def test_sharded_local_ba_rccl_two_ranks(mode):
    """The multi-rank RCCL transport itself: two fresh processes, one GPU each, a 2-rank communicator made by fb_rccl_*,
    ncclAllReduce between the kernels on the BA stream (out-of-place exchange 2, final pack / unpack, abort flag), against
    the oracle.  Skipped on a one-GPU box: until a box with two GPUs has run it, multi-rank RCCL is UNVERIFIED."""
    import fishbirdeyevisualslam_amd as fb
    if fb.lib().fb_device_count() < 2:   # counting devices does not initialise the GPU in this process
        pytest.skip("needs >= 2 GPUs (multi-rank RCCL stays unverified on this box)")
    outs = _run_world2(mode)
    assert all("rccl_ranks_seen=2" in o and "flags_equal=True" in o and "identical_across_ranks=True" in o for o in outs)


@pytest.mark.gpu
def test_sharded_local_ba_rccl_single_rank_vs_oracle():
    """The RCCL transport end to end on the one GPU of the box: a 1-rank communicator made through fb_rccl_*, the exchanges
    are real ncclAllReduce calls on the BA stream (identity for one rank).  Multi-rank arithmetic is covered by the
    world-2 tests above (same protocol, host transport)."""
    import ctypes as C
    import numpy as np
    import fishbirdeyevisualslam_amd as fb
    import oracle_lib as O
    from fishbirdeyevisualslam_amd import ba_problem, synth, dist as fbd
    L = fb.lib()
    comm = fbd.RcclComm(L, 0, 1)
    try:
        p = synth.make_ba_problem(4000, n_kf=8, n_mp=1200, n_mpb=300)
        a, out_s, keep = ba_problem.local_ba_args(p, with_odom=1)
        fbd.local_ba_sharded_rccl(L, a, 0, 1, comm)
        a1, out_1, keep1 = ba_problem.local_ba_args(p, with_odom=1)
        O.call("orc_local_ba", a1)
        for k in ("kf_Tcw", "mp_xw", "mpb_xw"):
            assert float(np.abs(out_s[k] - out_1[k]).max() / max(1.0, np.abs(out_1[k]).max())) <= 1e-4, k
        np.testing.assert_array_equal(out_s["obs_outlier"], out_1["obs_outlier"])
        np.testing.assert_array_equal(out_s["bobs_outlier"][: len(p["bobs_kf"])], out_1["bobs_outlier"][: len(p["bobs_kf"])])
    finally:
        comm.close()


@pytest.mark.gpu
def test_sharded_rccl_single_rank_hbm_resident_system():
    """30 key frames: the reduced system lives in HBM; the schedule is the device-resident one and exchange 1 of that path
    (the reduced system S | r) is an ncclAllReduce on the BA stream like the others."""
    import numpy as np
    import fishbirdeyevisualslam_amd as fb
    import oracle_lib as O
    from fishbirdeyevisualslam_amd import ba_problem, synth, dist as fbd
    L = fb.lib()
    comm = fbd.RcclComm(L, 0, 1)
    try:
        p = synth.make_ba_problem(4010, n_kf=30, n_fixed=2, n_mp=1500, n_mpb=300)
        a, out_s, keep = ba_problem.local_ba_args(p, with_odom=1)
        fbd.local_ba_sharded_rccl(L, a, 0, 1, comm)
        a1, out_1, keep1 = ba_problem.local_ba_args(p, with_odom=1)
        O.call("orc_local_ba", a1)
        for k in ("kf_Tcw", "mp_xw", "mpb_xw"):
            assert float(np.abs(out_s[k] - out_1[k]).max() / max(1.0, np.abs(out_1[k]).max())) <= 1e-4, k
        np.testing.assert_array_equal(out_s["obs_outlier"], out_1["obs_outlier"])
    finally:
        comm.close()
