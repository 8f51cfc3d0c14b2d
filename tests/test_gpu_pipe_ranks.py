"""The pipe's gather between ranks, with the passes of a sharded run in flight (havac_amd/csrc/havac_pipe.hip).

havac_pipe_collect gathers each pass to rank 0 while later passes run.  Two stream dependencies keep that right: a slot's next
pass waits for the slot's last gather (`s.gathered`: it overwrites the hit buffer that gather sends from), and the caller's
stream waits for the gather before it reads rank 0's list.  The stand-in of tests/native/rccl_standin.cpp completes an
operation inside the call, so by default neither dependency can be seen to fail; in its stream-ordered mode a call only
enqueues, a send reads its buffer when the stream gets there, and a bounded kernel in front of every operation keeps that
moment well behind the call.  2 and 3 processes share GPU 0, bound to the stand-in through use_gather_library, and drive
ShardedSsv on the C route (asserted on every rank) at five (depth, kernel streams) pairs, in both modes:

  S1  12 different passes (heights on both sides of 256, 5 ... 12 segments, one dense, one empty, one with hits in the last
      rank's columns only, totals that rise so every slot's receive buffer regrows with passes in flight): every list that
      collect() returned, cloned at once and re-read just before its slot is submitted again, equals the checker's;
  S2  an overflow in the last rank's shard between good passes: that rank raises its own error, the others ShardFailure
      naming it, every other pass equals the checker;
  S3  havac_pipe_run at (3, 2): its last list equals the checker's;
  S4  (stream mode) the records-stage deadline: wait_gathers() raises CollectiveTimeout naming rank, stage and 300 ms;
  S5  (stream mode) the stand-in really enqueues: right after havac_gather_records returns, the receive buffer still holds
      its pattern; after the wait it holds the list.

tests/pipe_rank_worker.py is one rank.
"""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from test_gpu_gather_ranks import build_standin

pytestmark = pytest.mark.gpu

CONFIGS = ["1,1", "2,1", "2,2", "3,2", "4,3"]


def run_ranks(tmp_path, world, mode):
    build_standin()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    worker = os.path.join(ROOT, "tests", "pipe_rank_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(tmp_path), mode], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=420)[0])
    finally:
        for p in procs:          # the exact processes this test started, nothing else
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r}:\n{logs[r][-3000:]}"
    return [json.load(open(tmp_path / f"result_{r}.json")) for r in range(world)]


@pytest.mark.parametrize("mode", ["sync", "stream"])
@pytest.mark.parametrize("world", [2, 3])
def test_pipe_gathers_every_pass_between_ranks(tmp_path, oracle, world, mode):
    res = run_ranks(tmp_path, world, mode)
    for r in res:
        assert r["version"] == 22203                          # the stand-in's number: that library really was the one bound
        assert r["lag_ms"] == (30 if mode == "stream" else 0)
    # S1: every pass at every (depth, kernel streams): rank 0's list and its re-read equal the checker's; every rank found its own
    for cfg in CONFIGS:
        depth, streams = map(int, cfg.split(","))
        for r in res:
            s1 = r["s1"][cfg]
            assert s1["c_route"], cfg
            assert all(s1["found_ok"]) and len(s1["found_ok"]) == 12, (cfg, r["rank"], s1["found_ok"])
            assert s1["streams_used"] == streams, cfg
        s1 = res[0]["s1"][cfg]
        assert s1["passes"] == 12 and all(s1["equal"]), (cfg, s1["equal"])
        assert s1["rereads"] == (12 - depth if depth > 1 else 0) and all(s1["reread_equal"]), (cfg, s1["reread_equal"])
    # S2: the overflowing pass fails on every rank -- its own error on the last rank, ShardFailure naming it elsewhere
    for cfg in ("3,2", "4,3"):
        for r in res:
            s2 = r["s2"][cfg]
            assert s2["c_route"] and s2["failed"]["pass"] == 2, (cfg, s2)
            if r["rank"] == world - 1:
                assert s2["failed"]["kind"] == "HitOverflowError", s2["failed"]
            else:
                assert s2["failed"]["kind"] == "ShardFailure" and f"rank(s) {world - 1}" in s2["failed"]["message"], s2["failed"]
            assert s2["found_ok"] == [True] * 4, (cfg, s2)
        assert res[0]["s2"][cfg]["lists"] == [True] * 4, (cfg, res[0]["s2"][cfg])
    # S3: havac_pipe_run's last list, for two loops of different inputs
    for r in res:
        assert r["s3"]["c_route"] and r["s3"]["found_ok"] == [True, True], r["s3"]
    assert res[0]["s3"]["equal"] == [True, True]
    if mode != "stream":
        return
    # S5: the stand-in enqueues: the receive buffer is untouched when the call returns, filled after the wait
    for r in res:
        assert r["s5"]["counts_ok"], r["s5"]
    s5 = res[0]["s5"]
    assert s5["pattern_before"] and s5["read_s"] < 0.8 and s5["list_after"], s5
    # S4: the records-stage deadline
    for k, r in enumerate(res):
        msg = r["s4"]["message"]
        assert f"rank {k} of {world}" in msg and "the gather of the records" in msg and "300 ms" in msg, msg
        assert 0.25 < r["s4"]["seconds"] < 1.4, r["s4"]
