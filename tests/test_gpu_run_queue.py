"""The run queue above the kernels against the checker: which hit list a caller receives and which inputs its records are
resolved against, under out-of-order waits, state queries, aborts, overflows, model and sequence reloads, with up to three
runs open (havac_dev_set_pipeline_depth / Havac::setPipelineDepth) and one or two device parts behind the handle.

A small pure-Python model of the documented semantics (RunQueue) says, for every call, which run it speaks of and what it
must return; seeded random call sequences are driven through the device layer (HavacHwClient) and the file level (Havac)
with it.  The invariant: no fetch ever returns a list other than the one the checker gives for THAT run's own inputs -- it
returns that list or raises the predicted error -- and the handle never gets stuck (after any sequence, draining every open
run and starting a fresh one gives a correct list).  Then one named regression per way the layers were found to go wrong,
and the pipe (havac_pipe_run, ShardedSsv) after a failed pass."""
import ctypes as C
import os
import random
import time

import numpy as np
import pytest

from havac_amd import synth
from oracle.resolve import expected_hits

pytestmark = pytest.mark.gpu

RUNNING, COMPLETED, ERROR, ABORT = 3, 4, 5, 6
LIBC = C.CDLL(None)


# ---- the model -----------------------------------------------------------------------------------------------------------

class Run:
    def __init__(self, inputs, overflows):
        self.inputs = inputs
        self.finished = False                     # the device layer has collected it (wait / state / abort / fetch / retire)
        self.outcomes = {"overflow" if overflows else "ok"}   # narrowed as calls observe it; "aborted": stopped by abort

    def states(self):
        s = set()
        for o in self.outcomes:
            s |= {"ok": {COMPLETED}, "overflow": {ERROR}, "aborted": {ABORT, ERROR}}[o]
        return s

    def observe_state(self, state):
        """narrows the outcomes to those that report `state`"""
        keep = {o for o in self.outcomes if state in {"ok": {COMPLETED}, "overflow": {ERROR}, "aborted": {ABORT, ERROR}}[o]}
        assert keep, f"state {state}, expected one of {sorted(self.states())}"
        self.outcomes = keep


class RunQueue:
    """Up to `depth` runs open; every call speaks of the oldest.  A new run needs a free slot: at depth 1 a finished run is
    closed by the next one, deeper the oldest is closed to make room if it is finished, else the new run is refused (logic
    error).  fetch_closes: a fetch at depth > 1 closes the run it returns or raises for (the file level)."""

    def __init__(self, depth, fetch_closes):
        self.depth, self.fetch_closes, self.runs = depth, fetch_closes, []

    def start(self, inputs, overflows):
        """-> True if the run must be accepted"""
        if len(self.runs) == self.depth:
            if not self.runs[0].finished:
                return False
            self.runs.pop(0)
        self.runs.append(Run(inputs, overflows))
        return True

    def oldest(self):
        return self.runs[0] if self.runs else None

    def finish(self, state):
        r = self.runs[0]
        r.observe_state(state)
        r.finished = True

    def abort(self, state):
        """the oldest run reported `state` after an abort.  If it had not finished, the device stopped every unfinished run --
        unless the oldest had completed already: it then reports COMPLETED, or ERROR if it overflowed.  When the oldest may
        overflow anyway, or may have been stopped by an earlier abort, its state does not say which happened: the other
        runs may or may not have been stopped"""
        r = self.runs[0]
        if not r.finished:
            if state == COMPLETED:
                stopped = False
            elif r.outcomes & {"overflow", "aborted"}:
                stopped = None
            else:
                stopped = True
            if stopped is not False:
                r.outcomes = r.outcomes | {"aborted"}
            for other in self.runs[1:]:
                if not other.finished and stopped is not False:
                    other.outcomes = {"aborted"} if stopped else other.outcomes | {"aborted"}
        self.finish(state)

    def closed_by_fetch(self):
        if self.fetch_closes and self.depth > 1:
            self.runs.pop(0)


def fetch_outcome(run, call):
    """call() -> its result, or the exception the run's outcome predicts: ('ok', value) / ('overflow', None) / ('aborted', None)"""
    from havac_amd.hw_client import HitOverflowError, LogicError
    try:
        value = call()
    except HitOverflowError:
        assert run.outcomes & {"overflow", "aborted"}, f"HitOverflowError, expected {sorted(run.outcomes)}"
        run.outcomes &= {"overflow", "aborted"}
        return "overflow", None
    except LogicError:
        assert "aborted" in run.outcomes, f"LogicError, expected {sorted(run.outcomes)}"
        run.outcomes = {"aborted"}
        return "aborted", None
    assert "ok" in run.outcomes, f"a list, expected {sorted(run.outcomes)}"
    run.outcomes = {"ok"}
    return "ok", value


def replayable(ops, body):
    """runs body(); on failure the operation list is printed so that the sequence can be replayed by hand"""
    try:
        body()
    except BaseException:
        print("operations:", ops)
        raise


# ---- the device layer (HavacHwClient) ------------------------------------------------------------------------------------

def device_inputs():
    seqs, models = [], []
    for j, nseg in enumerate((3, 5)):
        sym = synth.random_symbols(nseg * synth.SEGMENT, 40 + j)
        seqs.append(sym)
    for k, rows in enumerate((77, 300, 1500)):
        m, cons = synth.dfam_like_model(rows, 60 + k)
        for sym in seqs:
            synth.plant_homologs(sym, cons, sym.size, every=4000 + 700 * k, length=min(150, rows), seed=k)
        models.append(m)
    models.append(np.full((9, 4), 127, np.int8))              # a hit on every third row of every diagonal: overflows
    return seqs, models


DEVICE_OPS = ["writePhmm", "writeSequence", "invoke", "invoke", "invoke", "wait", "state", "abort", "getHitList", "getHitList",
              "retire"]


def drive_device(c, queue, ops, seqs, models, want, capacity, counts):
    from havac_amd.hw_client import LogicError
    cur = [0, 0]                                             # (sequence, model) written last
    c.writeSequence(synth.pack_2bit(seqs[0]))
    c.writePhmm(models[0])
    for op, arg in ops:
        r = queue.oldest()
        if op == "writePhmm":
            c.writePhmm(models[arg]); cur[1] = arg
        elif op == "writeSequence":
            c.writeSequence(synth.pack_2bit(seqs[arg])); cur[0] = arg
        elif op == "invoke":
            inputs = tuple(cur)
            if queue.start(inputs, want(inputs).size > capacity):
                c.invokeHavacSsvAsync()
            else:
                with pytest.raises(LogicError):
                    c.invokeHavacSsvAsync()
        elif r is None:
            with pytest.raises(RuntimeError):               # no open run: logic or runtime error, per the reference
                {"wait": c.waitForHavacSsvAsync, "state": c.getHwState, "abort": c.abort, "getHitList": c.getHitList,
                 "retire": c.retire}[op]()
        elif op == "wait":
            queue.finish(c.waitForHavacSsvAsync())
        elif op == "state":
            s = c.getHwState()
            if s != RUNNING:
                queue.finish(s)
            else:
                assert not r.finished
        elif op == "abort":
            queue.abort(c.abort())
        elif op == "getHitList":
            kind, got = fetch_outcome(r, c.getHitList)
            r.finished = True
            if kind == "ok":
                assert np.array_equal(got, want(r.inputs)), r.inputs
                counts["compared"] += 1
        elif op == "retire":
            c.retire()
            queue.runs.pop(0)
        assert c.openRuns() == len(queue.runs)
    # drain, then a fresh run is correct
    while queue.runs:
        c.retire()
        queue.runs.pop(0)
    c.writeSequence(synth.pack_2bit(seqs[1]))
    c.writePhmm(models[1])
    c.invokeHavacSsvAsync()
    assert np.array_equal(c.getHitList(), want((1, 1)))
    c.retire()
    counts["compared"] += 1


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_device_layer_random_call_orders(depth, parts, oracle):
    from havac_amd.hw_client import HavacHwClient
    seqs, models = device_inputs()
    cache = {}

    def want(inputs):
        if inputs not in cache:
            cache[inputs] = oracle.ssv_fast(seqs[inputs[0]], models[inputs[1]])
        return cache[inputs]

    normal = max(want((j, k)).size for j in range(2) for k in range(3))
    # one part: the dense model overflows, the others fit; two parts: each part has a buffer of its own, so the capacity only
    # says which runs overflow if it is large enough for every run
    capacity = normal + 64 if parts == 1 else 1 << 20
    assert parts == 2 or min(want((j, 3)).size for j in range(2)) > capacity
    counts = {"compared": 0}
    c = HavacHwClient(deviceIndices=[0] * parts)
    try:
        c.setHitCapacity(capacity)
        c.setPipelineDepth(depth)
        for seed in range(30):
            rng = random.Random(1000 * depth + 100 * parts + seed)
            ops = []
            for _ in range(40):
                op = rng.choice(DEVICE_OPS)
                ops.append((op, rng.randrange(2) if op == "writeSequence" else rng.randrange(4) if op == "writePhmm" else None))
            queue = RunQueue(depth, fetch_closes=False)
            replayable(ops, lambda: drive_device(c, queue, ops, seqs, models, want, capacity, counts))
    finally:
        c.close()
    print(f"device layer, depth {depth}, {parts} part(s): {counts['compared']} fetched runs equal to the checker")
    assert counts["compared"] >= 100


# ---- the file level (Havac) ----------------------------------------------------------------------------------------------

class FileInputs:
    """3 HMM files whose model lengths differ + 1 that overflows the hit buffer, 2 FASTAs with different record counts and
    lengths (ambiguity codes included); what a run must return given (FASTAs loaded so far, the srand seed of the last load,
    the HMM file)"""

    def __init__(self, tmp_path, oracle, boundary, both_strands):
        from oracle.cases import random_text
        rng = np.random.default_rng(17)
        self.dir, self.oracle, self.boundary, self.both = tmp_path, oracle, boundary, both_strands
        genome = rng.integers(0, 4, size=2000, dtype=np.uint8)      # every model's consensus is a stretch of it
        text = "".join("ACGT"[v] for v in genome)
        self.hmms = []
        for i, lengths in enumerate(([60, 300, 150], [220, 90], [33, 400, 75, 12], [24])):
            models = []
            for k, L in enumerate(lengths):
                cons = np.zeros(L, np.uint8) if i == 3 else genome[(37 * (i + 1) + 101 * k) % 1500:][:L]
                models.append(dict(name=f"m{i}_{k}", acc=f"RF{i}{k:04d}", emissions=synth.emissions_from_consensus(cons, 80 + 10 * i + k),
                                   maxl=3 * L + 50, mu=-9.2 + 0.1 * k, lam=0.71))
            self.hmms.append(os.path.join(str(tmp_path), f"h{i}.hmm"))
            synth.write_hmm(self.hmms[-1], models)          # h3: an A-only model that overflows the hit buffer on the A runs
        records = [[random_text(3000, rng) + text[:700] + "A" * 1500, random_text(5000, rng) + text[900:1700], "ACGTA" * 3],
                   [random_text(100, rng), "NNNNRYKM" + text[300:1200] + "A" * 2000, "C", random_text(2000, rng) + text[1500:],
                    random_text(700, rng)]]
        self.fastas = []
        for j, recs in enumerate(records):
            self.fastas.append(os.path.join(str(tmp_path), f"f{j}.fa"))
            synth.write_fasta(self.fastas[-1], [(f"f{j}_{n}", t) for n, t in enumerate(recs)])
        self.texts = [open(f).read() for f in self.fastas]
        self._cache = {}

    def lengths(self, loaded):
        from oracle.cases import records_of
        out = []
        for j in loaded:
            out += [len(t) for t in records_of(self.fastas[j])]
        return out

    def raw(self, inputs):
        """-> (raw records in device order, model lengths)"""
        from havac_amd import havac
        from oracle.cases import boundary_raw
        if inputs not in self._cache:
            loaded, seed, k = inputs
            fa = os.path.join(str(self.dir), "cat_" + "_".join(map(str, loaded)) + ".fa")
            with open(fa, "w") as f:
                f.write("".join(self.texts[j] for j in loaded))
            if self.boundary:
                raw, lens = boundary_raw(fa, self.hmms[k], 0.02, self.oracle, self.both)
            else:
                packed, _, _ = havac.pack_fasta_layout(fa, False, self.both, seed=seed)
                table, lens = havac.project_hmm(self.hmms[k], 0.02)
                raw = self.oracle.ssv_fast(self.oracle.unpack_2bit(packed), table)
            self._cache[inputs] = (raw, lens)
        return self._cache[inputs]

    def hits(self, inputs):
        from havac_amd import havac
        raw, lens = self.raw(inputs)
        return [havac.HavacHit(*h) for h in expected_hits(raw, self.lengths(inputs[0]), lens, boundary=self.boundary,
                                                          both_strands=self.both)]

    def windows(self, inputs, flank):
        from havac_amd import havac
        _, lens = self.raw(inputs)
        return havac.merge_windows(self.hits(inputs), lens, self.lengths(inputs[0]), flank)


FILE_OPS = ["loadPhmm", "loadPhmm", "loadSequence", "run", "run", "run", "wait", "state", "abort", "getHits", "getHits", "getWindows"]
MAX_SEQUENCE_LOADS = 3          # loadSequence appends (FastaVector, as the reference): the sequence grows with every load


def drive_file(h, queue, ops, files, capacity, counts):
    from havac_amd.hw_client import LogicError
    loaded, seed, hmm = [0], 0, 0
    LIBC.srand(seed)
    h.loadSequence(files.fastas[0])
    h.loadPhmm(files.hmms[0])

    def check_fetch(r, call, windows=None):
        kind, got = fetch_outcome(r, call)
        r.finished = True
        if kind == "ok":
            if windows is None:
                assert got == files.hits(r.inputs), r.inputs
            else:
                assert got == files.windows(r.inputs, windows), r.inputs
            assert np.array_equal(h.rawHits(), files.raw(r.inputs)[0]), r.inputs
            counts["compared"] += 1
        queue.closed_by_fetch()

    for op, arg in ops:
        r = queue.oldest()
        if op == "loadPhmm":
            h.loadPhmm(files.hmms[arg]); hmm = arg
        elif op == "loadSequence":
            if len(loaded) < MAX_SEQUENCE_LOADS:
                seed = 100 + arg
                LIBC.srand(seed)
                h.loadSequence(files.fastas[arg]); loaded.append(arg)
        elif op == "run":
            inputs = (tuple(loaded), seed, hmm)
            if queue.start(inputs, files.raw(inputs)[0].size > capacity):
                h.runHardwareClientAsync()
            else:
                with pytest.raises(LogicError):
                    h.runHardwareClientAsync()
        elif r is None:
            with pytest.raises(RuntimeError):
                {"wait": h.waitHardwareClientAsync, "state": h.currentHardwareState, "abort": h.abortHardwareClient,
                 "getHits": h.getHitsFromFinishedRun, "getWindows": h.getWindowsFromFinishedRun}[op]()
        elif op == "wait":
            h.waitHardwareClientAsync()
            queue.finish(h.currentHardwareState())
        elif op == "state":
            s = h.currentHardwareState()
            if s != RUNNING:
                queue.finish(s)
        elif op == "abort":
            h.abortHardwareClient()
            queue.abort(h.currentHardwareState())           # (the oldest run has been finished by the abort: its final state)
        elif op == "getHits":
            check_fetch(r, h.getHitsFromFinishedRun)
        elif op == "getWindows":
            check_fetch(r, lambda: h.getWindowsFromFinishedRun(arg), windows=arg)
    # drain every open run (each fetch is checked), then a fresh run is correct
    if queue.depth > 1:
        while queue.runs:
            check_fetch(queue.oldest(), h.getHitsFromFinishedRun)
    else:
        if queue.runs and not queue.runs[0].finished:
            h.waitHardwareClientAsync()
            queue.finish(h.currentHardwareState())
        queue.runs = []
    h.loadPhmm(files.hmms[1])
    inputs = (tuple(loaded), seed, 1)
    assert queue.start(inputs, False)
    h.runHardwareClientAsync()
    check_fetch(queue.oldest(), h.getHitsFromFinishedRun)
    if queue.depth == 1:
        queue.runs = []


@pytest.mark.parametrize("depth,boundary,both_strands", [(1, False, False), (2, False, False), (3, False, False), (2, True, True)])
def test_file_level_random_call_orders(depth, boundary, both_strands, tmp_path, oracle):
    from havac_amd import havac
    files = FileInputs(tmp_path, oracle, boundary, both_strands)
    loads = [[0]] + [[0, a] for a in range(2)] + [[0, a, b] for a in range(2) for b in range(2)]
    reachable = [(tuple(l), 100 + l[-1] if len(l) > 1 else 0, k) for l in loads for k in range(4)]
    sizes = {x: files.raw(x)[0].size for x in reachable}
    normal = max(v for x, v in sizes.items() if x[2] < 3)
    dense = min(v for x, v in sizes.items() if x[2] == 3)
    assert dense > normal + 64 and min(v for x, v in sizes.items() if x[2] < 3) > 20, (dense, normal)
    capacity = normal + 32
    counts = {"compared": 0}
    for seed in range(30):
        rng = random.Random(7000 + 100 * depth + 10 * boundary + seed)
        ops = []
        for _ in range(40):
            op = rng.choice(FILE_OPS)
            ops.append((op, rng.randrange(4) if op == "loadPhmm" else rng.randrange(2) if op == "loadSequence"
                        else rng.choice([0, 30]) if op == "getWindows" else None))
        queue = RunQueue(depth, fetch_closes=True)
        h = havac.Havac(0, 0.02)        # a fresh handle per seed: loadSequence appends, the sequence grows with every load
        try:
            h.setBoundaryMode(boundary)
            h.setBothStrands(both_strands)
            h.setHitCapacity(capacity)
            h.setPipelineDepth(depth)
            replayable(ops, lambda: drive_file(h, queue, ops, files, capacity, counts))
        finally:
            h.close()
    name = f"file depth {depth}" + (", boundary mode, both strands" if boundary else "")
    print(f"file level, {name}: {counts['compared']} fetched runs equal to the checker")
    assert counts["compared"] >= 100


# ---- named regressions ---------------------------------------------------------------------------------------------------

def fresh_havac(files, depth, capacity=None):
    from havac_amd import havac
    h = havac.Havac(0, 0.02)
    h.setBoundaryMode(files.boundary)
    h.setBothStrands(files.both)
    if capacity:
        h.setHitCapacity(capacity)
    h.setPipelineDepth(depth)
    return h


@pytest.mark.parametrize("finish_with", ["wait", "state", "abort"])
def test_a_run_closed_to_make_room_takes_its_models_with_it(finish_with, tmp_path, oracle):
    """Depth 2: run A, run B, A finished (wait / a state query / an abort that finds it complete) but not fetched, loadPhmm,
    run C -- the device layer closes A to make room.  B's hits must be resolved against B's models.  Unfixed symptom: B's
    records resolved against A's prefix sums (wrong phmmIndex / phmmPosition)."""
    files = FileInputs(tmp_path, oracle, False, False)
    h = fresh_havac(files, 2)
    try:
        LIBC.srand(0)
        h.loadSequence(files.fastas[0])
        h.loadPhmm(files.hmms[0]); h.runHardwareClientAsync()          # A
        h.loadPhmm(files.hmms[1]); h.runHardwareClientAsync()          # B
        if finish_with == "wait":
            h.waitHardwareClientAsync()
        elif finish_with == "state":
            deadline = time.time() + 30
            while h.currentHardwareState() == RUNNING and time.time() < deadline:
                time.sleep(0.001)
        else:
            time.sleep(0.5)                                             # (A is a few milliseconds of GPU work: complete by now)
            h.abortHardwareClient()
        assert h.currentHardwareState() == COMPLETED
        h.loadPhmm(files.hmms[2]); h.runHardwareClientAsync()          # C: A is closed to make room
        b = ((0,), 0, 1)
        want = files.hits(b)
        assert {x.phmmIndex for x in want} == {0, 1}
        assert h.getHitsFromFinishedRun() == want                       # B
        assert h.getHitsFromFinishedRun() == files.hits(((0,), 0, 2))   # C
    finally:
        h.close()


def test_a_failed_run_is_closed_by_its_fetch(tmp_path, oracle):
    """Depth 2: a run that overflows, then a good one.  The overflowed run's fetch raises and closes it; the next fetch is
    the good run's.  Unfixed symptom: HitOverflowError again on the run after the overflowed one."""
    from havac_amd.hw_client import HitOverflowError
    files = FileInputs(tmp_path, oracle, False, False)
    good, dense = ((0,), 0, 0), ((0,), 0, 3)
    capacity = files.raw(good)[0].size + 16
    assert files.raw(dense)[0].size > capacity
    h = fresh_havac(files, 2, capacity)
    try:
        LIBC.srand(0)
        h.loadSequence(files.fastas[0])
        h.loadPhmm(files.hmms[3]); h.runHardwareClientAsync()
        h.loadPhmm(files.hmms[0]); h.runHardwareClientAsync()
        with pytest.raises(HitOverflowError):
            h.getHitsFromFinishedRun()
        assert h.rawHits().size == 0                                    # (no list of an earlier fetch is left behind)
        assert h.getHitsFromFinishedRun() == files.hits(good)
        h.runHardwareClientAsync()
        assert h.getWindowsFromFinishedRun(5) == files.windows(good, 5)
    finally:
        h.close()


@pytest.mark.parametrize("boundary,both_strands", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("depth", [1, 2])
def test_loading_a_sequence_leaves_the_open_runs_alone(depth, boundary, both_strands, tmp_path, oracle):
    """Run A on FASTA 1, then loadSequence(FASTA 2) before A's hits are fetched: A's hits and windows are resolved against
    the records A ran on.  Unfixed symptom: A's records resolved against FASTA 1 + 2 (hits in the padding behind FASTA 1 become
    hits of FASTA 2's records; with both strands the second half starts at another column)."""
    files = FileInputs(tmp_path, oracle, boundary, both_strands)
    a = ((0,), 0, 3)
    h = fresh_havac(files, depth)
    try:
        LIBC.srand(0)
        h.loadSequence(files.fastas[0])
        h.loadPhmm(files.hmms[3])
        h.runHardwareClientAsync()
        h.waitHardwareClientAsync()
        LIBC.srand(101)
        h.loadSequence(files.fastas[1])
        if depth == 1:
            assert h.getHitsFromFinishedRun() == files.hits(a)
            assert np.array_equal(h.rawHits(), files.raw(a)[0])
            assert h.getWindowsFromFinishedRun(3) == files.windows(a, 3)
        else:
            h.runHardwareClientAsync()                                  # B on FASTA 1 + 2
            assert h.getWindowsFromFinishedRun(3) == files.windows(a, 3)
            assert h.getHitsFromFinishedRun() == files.hits(((0, 1), 101, 3))
    finally:
        h.close()


@pytest.mark.parametrize("depth", [1, 2])
def test_setting_the_same_depth_keeps_the_open_runs_records(depth, tmp_path, oracle):
    """setPipelineDepth with the depth the handle already has leaves finished runs open (the device layer changes nothing), so
    their records stay too.  Run A, wait, loadPhmm(other), setPipelineDepth(same), (depth 2: run B): A's hits are resolved
    against A's models.  Unfixed symptom: A's records resolved against the models loaded since (or B's)."""
    files = FileInputs(tmp_path, oracle, False, False)
    h = fresh_havac(files, depth)
    try:
        LIBC.srand(0)
        h.loadSequence(files.fastas[0])
        h.loadPhmm(files.hmms[0])
        h.runHardwareClientAsync()
        h.waitHardwareClientAsync()
        h.loadPhmm(files.hmms[1])
        h.setPipelineDepth(depth)
        if depth > 1:
            h.runHardwareClientAsync()
        assert h.getHitsFromFinishedRun() == files.hits(((0,), 0, 0))
        if depth > 1:
            assert h.getHitsFromFinishedRun() == files.hits(((0,), 0, 1))
    finally:
        h.close()


# ---- aborts that stop runs in flight -------------------------------------------------------------------------------------
# The long run of test_runs_in_flight_behind_the_handle: 60,000 rows x 2,000 segments, ~1.5e12 cells (tens of milliseconds of
# GPU work), so that the abort a few calls after its start finds it running.  Its own list is never needed: it is stopped.
# Before it, one short run per slot on the same sequence, checked against the checker: a slot's first pass on a sequence that
# size grows its buffers, which waits for what its stream still holds -- at depth 3 the third slot shares the long run's
# stream, and its first pass would wait for the long run to complete.

LONG_ROWS, LONG_SEGMENTS = 60_000, 2000
LONG_CAPACITY = 1 << 27          # (a stopped sweep may still have queued many records)


@pytest.mark.parametrize("depth", [2, 3])
def test_device_layer_abort_stops_every_run_in_flight(depth, oracle):
    """The long run A, short runs behind it, abort: A reports ABORT, its list and the lists of the runs behind it raise
    LogicError (the model predicts it), retire closes them one by one, and a fresh run equals the checker."""
    from havac_amd.hw_client import HavacHwClient
    long_model, _ = synth.dfam_like_model(LONG_ROWS, 1)
    short, _ = synth.dfam_like_model(77, 99)
    seqs, models = device_inputs()
    c = HavacHwClient()
    try:
        c.setHitCapacity(LONG_CAPACITY)
        c.setPipelineDepth(depth)
        queue = RunQueue(depth, fetch_closes=False)
        packed = synth.random_packed(LONG_SEGMENTS * synth.SEGMENT, 2)
        c.writeSequence(packed)
        c.writePhmm(short)
        want_short = oracle.ssv_fast(oracle.unpack_2bit(packed), short)
        for _ in range(depth):
            c.invokeHavacSsvAsync()
            assert np.array_equal(c.getHitList(), want_short)
            c.retire()
        c.writePhmm(long_model)
        c.invokeHavacSsvAsync()
        assert queue.start("long", False)
        c.writePhmm(short)                                    # (waits until A has read its model)
        for k in range(depth - 1):
            c.invokeHavacSsvAsync()
            assert queue.start(f"short {k}", False)
        assert c.openRuns() == depth
        state = c.abort()
        assert state == ABORT, "the long run had completed before the abort: nothing was stopped"
        queue.abort(state)
        assert all(r.outcomes == {"aborted"} for r in queue.runs)
        while queue.runs:
            r = queue.oldest()
            queue.finish(c.waitForHavacSsvAsync())
            assert fetch_outcome(r, c.getHitList)[0] == "aborted"        # LogicError, as the model predicts
            c.retire()
            queue.runs.pop(0)
            assert c.openRuns() == len(queue.runs)
        c.writeSequence(synth.pack_2bit(seqs[1]))
        c.writePhmm(models[1])
        c.invokeHavacSsvAsync()
        assert np.array_equal(c.getHitList(), oracle.ssv_fast(seqs[1], models[1]))
    finally:
        c.close()


@pytest.mark.parametrize("depth", [2, 3])
def test_file_level_abort_stops_every_run_in_flight(depth, tmp_path, oracle):
    """Havac: the long run A, short runs behind it (after loadPhmm of a short model file), abortHardwareClient.  A reports
    ABORT; fetching A raises LogicError and closes A; every run behind it reports ABORT and its fetch raises LogicError and
    closes it; then a fresh run equals the checker.  (Unfixed: A stays open after its fetch raises, and every later fetch
    raises for A.)"""
    from havac_amd import havac
    from havac_amd.hw_client import LogicError
    files = FileInputs(tmp_path, oracle, False, False)
    sym = synth.random_symbols(LONG_SEGMENTS * synth.SEGMENT - 4096, 2, pad=False)
    long_fa, long_hmm = str(tmp_path / "long.fa"), str(tmp_path / "long.hmm")
    synth.write_fasta(long_fa, [("long", sym)], width=10_000)
    _, cons = synth.dfam_like_model(LONG_ROWS, 1)
    synth.write_hmm(long_hmm, [dict(name="long", acc="RF99999", emissions=synth.emissions_from_consensus(cons, 5),
                                    maxl=3 * LONG_ROWS, mu=-9.2, lam=0.71)])
    h = fresh_havac(files, depth, LONG_CAPACITY)
    try:
        queue = RunQueue(depth, fetch_closes=True)
        LIBC.srand(3)
        h.loadSequence(long_fa)
        packed, _, _ = havac.pack_fasta(long_fa, seed=3)
        table, lens = havac.project_hmm(files.hmms[1], 0.02)
        raw = oracle.ssv_fast(oracle.unpack_2bit(packed), table)
        want = [havac.HavacHit(*x) for x in expected_hits(raw, [sym.size], lens)]
        assert len(want) > 20
        h.loadPhmm(files.hmms[1])
        for _ in range(depth):
            h.runHardwareClientAsync()
            assert h.getHitsFromFinishedRun() == want
        h.loadPhmm(long_hmm)
        h.runHardwareClientAsync()
        assert queue.start("long", False)
        h.loadPhmm(files.hmms[1])                             # (waits until A has read its model)
        for k in range(depth - 1):
            h.runHardwareClientAsync()
            assert queue.start(f"short {k}", False)
        h.abortHardwareClient()
        state = h.currentHardwareState()
        assert state == ABORT, "the long run had completed before the abort: nothing was stopped"
        queue.abort(state)
        assert all(r.outcomes == {"aborted"} for r in queue.runs)
        while queue.runs:
            r = queue.oldest()
            h.waitHardwareClientAsync()                       # the oldest open run: A, then each run behind it
            queue.finish(h.currentHardwareState())
            assert fetch_outcome(r, h.getHitsFromFinishedRun)[0] == "aborted"   # LogicError, as the model predicts
            queue.closed_by_fetch()
        with pytest.raises(LogicError):
            h.currentHardwareState()                          # every run is closed
        h.runHardwareClientAsync()                            # a fresh run: the long file, the short models
        assert h.getHitsFromFinishedRun() == want
        assert np.array_equal(h.rawHits(), raw)
    finally:
        h.close()


def _sharded_inputs(oracle):
    import torch
    sym = synth.random_symbols(4 * synth.SEGMENT, 9)
    good, cons = synth.dfam_like_model(300, 10)
    synth.plant_homologs(sym, cons, sym.size, every=5000, length=200)
    dense = np.full((9, 4), 127, np.int8)
    dev = torch.device("cuda", 0)
    d_seq = torch.from_numpy(synth.pack_2bit(sym)).to(dev)
    return sym, good, dense, dev, d_seq, (lambda m: torch.from_numpy(np.ascontiguousarray(m).reshape(-1)).to(dev))


def test_the_pipe_is_idle_after_a_failed_run_many(oracle):
    """ShardedSsv.run_many(3, dense model) overflows.  Afterwards nothing is in flight, in the pipe or in its Python mirror,
    and the engine is usable: run_many(4, good model) returns 4 timings and the checker's records, run() too.  havac_pipe_run
    refuses to start while a pass submitted by submit() is in flight, and that pass still collects the checker's list.
    Unfixed symptoms: stale passes in flight after the failure (collected by the next run_many, whose timing arrays are then
    written past their end -- here they have `depth` spare entries holding a sentinel, so the overrun shows as a failed
    assertion), and havac_pipe_run collecting the caller's pass."""
    import torch
    from havac_amd import _lib
    from havac_amd.dist import ShardedSsv
    from havac_amd.hw_client import HitOverflowError
    sym, good, dense, dev, d_seq, to_dev = _sharded_inputs(oracle)
    want = oracle.ssv_fast(sym, good)
    assert 50 < want.size < 4096 < oracle.ssv_fast(sym, dense).size
    depth = 2
    engine = ShardedSsv(4096, dev, depth=depth)
    L = _lib.load()
    try:
        d_good, d_dense = to_dev(good), to_dev(dense)
        with pytest.raises(HitOverflowError):
            engine.run_many(3, d_seq, sym.size, d_dense, dense.shape[0])
        assert L.havac_pipe_in_flight(engine._h) == 0 and engine.in_flight == []
        (records, found), timings = engine.run_many(4, d_seq, sym.size, d_good, good.shape[0])
        assert len(timings) == 4 and found == want.size
        assert np.array_equal(records.cpu().numpy().view(np.uint64), want)
        records, found = engine.run(d_seq, sym.size, d_good, good.shape[0])
        assert np.array_equal(records.cpu().numpy().view(np.uint64), want)
        # havac_pipe_run with a pass of the caller's in flight
        engine.submit(d_seq, sym.size, d_good, good.shape[0])
        nsteps, sentinel = 2, -12345.0
        k_ms, t_ms = (C.c_float * (nsteps + depth))(), (C.c_float * (nsteps + depth))()
        for i in range(nsteps + depth):
            k_ms[i] = t_ms[i] = sentinel
        f, p, n = C.c_uint64(0), C.c_void_p(), C.c_uint64(0)
        torch.cuda.synchronize(dev)
        rc = L.havac_pipe_run(engine._h, nsteps, d_seq.data_ptr(), sym.size, d_dense.data_ptr(), dense.shape[0], 0, 1, None,
                              k_ms, t_ms, C.byref(f), C.byref(p), C.byref(n))
        assert [k_ms[i] for i in range(nsteps, nsteps + depth)] == [sentinel] * depth
        assert [t_ms[i] for i in range(nsteps, nsteps + depth)] == [sentinel] * depth
        assert rc == _lib.E_LOGIC
        assert L.havac_pipe_in_flight(engine._h) == 1 and engine.in_flight != []
        records, found = engine.collect()
        assert np.array_equal(records.cpu().numpy().view(np.uint64), want)
    finally:
        torch.cuda.synchronize(dev)
        if L.havac_pipe_in_flight(engine._h) == 0:
            engine.release()
        engine.close()


def test_a_released_engine_refuses_its_contexts(oracle):
    """After ShardedSsv.release() the slots' contexts are freed: engine.ctx.last_ms() raises instead of handing the library
    a freed context.  Unfixed symptom: the call reaches the library with the freed handle."""
    from havac_amd.dist import ShardedSsv
    sym, good, _, dev, d_seq, to_dev = _sharded_inputs(oracle)
    engine = ShardedSsv(1 << 16, dev, depth=2)
    try:
        engine.run(d_seq, sym.size, to_dev(good), good.shape[0])
        assert engine.ctx.last_ms()[0] > 0
        engine.release()
        with pytest.raises(RuntimeError, match="closed|released"):
            engine.ctx.last_ms()
        for k in range(2):
            with pytest.raises(RuntimeError):
                engine._contexts[k].last_ms()
    finally:
        engine.close()
