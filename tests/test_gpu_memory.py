"""Device memory comes back: handles and pipes that are made, grown and destroyed again and again leave the GPU's free memory
where it was.  Every cycle allocates far more than the tolerance (hit buffers, text staging, grown sequence and ordering
buffers), so a cycle that kept any of it would show."""
import numpy as np
import pytest

from havac_amd import synth

pytestmark = pytest.mark.gpu

CYCLES = 3
TOLERANCE = 64 << 20


def _inputs():
    model, cons = synth.dfam_like_model(300, 11)
    sym = synth.random_symbols(360 * synth.SEGMENT, 12)        # 1.08 MB packed: enough to be page-locked for two parts
    synth.plant_homologs(sym, cons, sym.size, every=9000, length=200)
    chars = np.frombuffer(b"ACGT", np.uint8)[sym]
    ends = np.array([sym.size // 3, sym.size // 3 + 17, sym.size], np.uint64)
    return model, sym, chars, ends


def _handle_cycle(model, sym, chars, ends):
    """Two parts on one GPU, three runs in flight: every buffer the handle, its pipes and their contexts own, grown."""
    from havac_amd.hw_client import HavacHwClient
    c = HavacHwClient(deviceIndices=[0, 0])
    try:
        c.setHitCapacity(1 << 22)
        c.setPipelineDepth(3)
        c.writePhmm(model)

        def run():
            c.invokeHavacSsvAsync()
            c.waitForHavacSsvAsync()
            hits = c.getHitList()
            c.retire()
            return hits

        starts = c.writeSequenceRecords(chars, ends)                        # sequence, mask, temporaries
        c.appendReverseStrand(starts, np.diff(np.concatenate([[0], ends])).astype(np.uint64))      # grown, keeping the forward half
        assert run().size > 0
        c.writeSequenceChars(chars, [5, 70000], [1, 2])                      # text staging, patch temporaries
        assert run().size > 0
        c.writeSequence(synth.pack_2bit(sym))                               # column windows, page-locked source
        c.setTuning(-1, -1, -1, 0)                                          # the radix sort: its temporary and second buffer
        assert run().size > 0
    finally:
        c.close()


def _pipe_cycle(torch, dev, model, sym):
    """A pipe three deep, released (its last records kept) and destroyed."""
    from havac_amd.dist import ShardedSsv
    d_seq = torch.from_numpy(synth.pack_2bit(sym)).to(dev)
    d_phmm = torch.from_numpy(model.reshape(-1)).to(dev)
    eng = ShardedSsv(1 << 22, dev, depth=3)
    try:
        (_, found), _ = eng.run_many(5, d_seq, sym.size, d_phmm, model.shape[0])
        assert found > 0
        eng.release()
    finally:
        eng.close()
    del d_seq, d_phmm
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()


def test_handles_and_pipes_give_their_memory_back():
    import torch
    dev = torch.device("cuda", 0)
    model, sym, chars, ends = _inputs()

    def cycle():
        _handle_cycle(model, sym, chars, ends)
        _pipe_cycle(torch, dev, model, sym)
        torch.cuda.synchronize(dev)
        return torch.cuda.mem_get_info(dev)[0]

    start = cycle()          # (once first: what the runtime sets up on first use stays)
    for k in range(CYCLES):
        free = cycle()
        assert start - free < TOLERANCE, f"cycle {k + 1}: {(start - free) / 2**20:.1f} MiB less free device memory than after the first"
