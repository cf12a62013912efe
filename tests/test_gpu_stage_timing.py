"""What the read mapper's stages leave in the context's timing record (mgl_sw_ctx_get_timing), on the GPU.  Six stages have no
MGL_SW_KERNEL_* id -- seed, seed_strands, seed_index, chain_anchors, select_strand, rank_chains --: behind each the record is reset as
by every device entry and keeps the fill_kernel it had, and under mgl_sw_ctx_set_profiling(3) a stage between two alignment calls
leaves their running sum alone (ctx_return_workspace with kKeepFillKernel, mgl_amd/csrc/sw_ctx_access.h).

Shapes: two reads of 200 bases against windows of 300, k = 15, w = 10, an index over a reference of 2 000 bases.

The empty batch (n = 0) of seed_device and chain_anchors_device is here too; that of the other stage forms is in their own files:
test_gpu_seed_strands.py, test_gpu_seed_index.py, test_gpu_select_strand.py, test_gpu_rank_chains.py, test_gpu_describe.py and
test_gpu_locate_window.py."""
import pytest

torch = pytest.importorskip("torch")
from mgl_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

K, W = 15, 10


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


@pytest.fixture(scope="module")
def world(aligner):
    """-> (the pairs' device tensors and bounds, the seeds' tensors, the index): read p is ref[at:at + 200], its window ref[at - 50:at + 250]"""
    from mgl_amd.smithwaterman import _pack_pairs

    dev = torch.device("cuda", 0)
    ref = synth.random_genome(synth.rng_for(7), 2000)
    at = (300, 1200)
    windows, reads = [ref[a - 50:a + 250].tobytes() for a in at], [ref[a:a + 200].tobytes() for a in at]
    _, packed, _ = _pack_pairs(windows, reads, dev, None, False)
    seeds = tuple(torch.tensor([v, v], dtype=torch.int32, device=dev) for v in (50, 0, 20))  # window[50:70] is read[0:20]
    index = aligner.build_index(ref.tobytes(), K, W)
    yield packed, seeds, index
    index.close()


def _extend_seed(aligner, packed, seeds):
    out = aligner.extend_seed_device(*packed[:6], *seeds, *packed[6:], 32, -1)
    t = aligner.timing()
    assert (t.fill_kernel, t.dp_launches) == (13, 2)  # MGL_SW_KERNEL_EXTEND, a launch per side
    return out


def test_a_stage_without_a_kernel_id_keeps_fill_kernel_and_resets_the_rest(aligner, world):
    packed, seeds, index = world
    reads = packed[3:6]
    aln = _extend_seed(aligner, packed, seeds)

    def kept(name):
        t = aligner.timing()
        assert (t.fill_kernel, t.dp_launches) == (13, 0), name

    seeded = aligner.seed_device(*packed[:6], K, W)
    kept("seed")
    stranded = aligner.seed_strands_device(*packed[:6], K, W)
    kept("seed_strands")
    rows = aligner.seed_index_device(index, *reads)
    kept("seed_index")
    chain = aligner.chain_anchors_device(rows[4], rows[5], *rows[:4], 4096, dp=True)
    kept("chain_anchors")
    chosen = aligner.select_strand_device(*reads, *chain[:5])
    kept("select_strand")
    ranked = aligner.rank_chains_device(rows[5], *rows[:4], chain[5], chain[6], chain[7], 2, 4096, 4, 40, 1)  # (an exact read is one merged anchor)
    kept("rank_chains")
    torch.cuda.synchronize()
    # the stages did their work: both reads aligned end to end, seeded on the forward row of each form, chained, chosen, ranked
    assert aln[5].tolist() == [0, 0] and aln[0][:, 3:5].tolist() == [[0, 200], [0, 200]]
    assert seeded[4].tolist() == [0, 0] and int(seeded[0][2]) > 0
    assert stranded[6].tolist() == [0] * 4 and int(stranded[0][1]) > 0
    assert rows[6].tolist() == [0] * 4 and int(rows[0][1]) > 0
    assert chain[7][0::2].tolist() == [0, 0] and (chain[4][0::2] > 0).all() and chosen[0].tolist() == [0, 0]
    assert ranked[6].tolist() == [0, 0] and (ranked[0] >= 1).all()


def test_a_stage_between_two_calls_leaves_the_running_sum_of_profiling_3_alone(aligner, world):
    packed, seeds, _ = world
    aligner.set_profiling(3)
    try:
        _ = aligner.timing()  # (a new sum)
        aligner.extend_seed_device(*packed[:6], *seeds, *packed[6:], 32, -1)
        aligner.seed_device(*packed[:6], K, W)
        aligner.extend_seed_device(*packed[:6], *seeds, *packed[6:], 32, -1)
        t = aligner.timing()
        assert (t.fill_kernel, t.dp_launches) == (13, 4)  # two sides per call, both calls
        assert aligner.timing().dp_launches == 0  # (read and cleared)
    finally:
        aligner.set_profiling(0)
        torch.cuda.synchronize()


def test_the_empty_batch_of_seed_and_chain_anchors(aligner):
    dev = torch.device("cuda", 0)
    e = lambda dt: torch.empty(0, dtype=dt, device=dev)  # noqa: E731
    seeded = aligner.seed_device(e(torch.uint8), e(torch.int64), e(torch.int32), e(torch.uint8), e(torch.int64), e(torch.int32), K, W)
    assert [tuple(x.shape) for x in seeded] == [(1,), (0,), (0,), (0,), (0,)]
    chain = aligner.chain_anchors_device(e(torch.int32), e(torch.int32), seeded[0], *seeded[1:4], 0, dp=True)
    assert [None if x is None else tuple(x.shape) for x in chain] == [(1,)] + [(0,)] * 7
    torch.cuda.synchronize()
    assert seeded[0].dtype == chain[0].dtype == torch.int64 and int(seeded[0][0]) == 0 and int(chain[0][0]) == 0
