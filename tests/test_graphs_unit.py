"""DecodeGraphs bucket logic and the DecodeState buffers (pure; capture
itself is GPU-tested via the engine)."""
import torch

from bee2bee_amd.engine.graphs import DecodeGraphs, decode_slot_mapping


class _DummyRunner:
    device = torch.device("cpu")


def _graphs(max_batch):
    return DecodeGraphs(_DummyRunner(), max_batch, max_blocks_per_seq=4)


def test_buckets_cover_power_of_two_and_max():
    g = _graphs(48)
    assert g.buckets() == [1, 2, 4, 8, 16, 32, 48]
    assert g.bucket_for(1) == 1
    assert g.bucket_for(3) == 4
    assert g.bucket_for(33) == 48
    assert g.bucket_for(48) == 48
    assert g.bucket_for(500) == 48  # clamped


def test_buckets_exact_power_of_two():
    g = _graphs(64)
    assert g.buckets()[-1] == 64
    assert g.bucket_for(64) == 64
    assert g.bucket_for(17) == 32


def test_decode_slot_mapping_matches_python():
    bt = torch.tensor([[3, 7, 1], [5, 0, 0]], dtype=torch.int32)
    pos = torch.tensor([33, 2], dtype=torch.int32)
    slots = decode_slot_mapping(bt, pos, 32)
    # seq0: pos 33 -> block idx 1 (=7), offset 1 -> 7*32+1
    # seq1: pos 2  -> block idx 0 (=5), offset 2 -> 5*32+2
    assert slots.tolist() == [7 * 32 + 1, 5 * 32 + 2]


# ---- DecodeState: the decode inputs and the rebuild-or-bump rule ----------
# Page size 4, max_batch 8 and B = 3 are the smallest values with a live pad
# row (bucket 4) and a page-boundary crossing within two steps.

PAGE, MAX_B, WIDTH = 4, 8, 4
SEQS, SCRATCH = [10, 11, 12], -1
LAST, LENGTHS = [5, 6, 7], [2, 4, 9]


def _kv():
    from bee2bee_amd.engine.kv import PagedKV
    from bee2bee_amd.models.spec import PRESETS

    kv = PagedKV(PRESETS["tiny"], torch.device("cpu"), torch.float32,
                 n_blocks=16, block_size=PAGE)
    kv.new_seq(SCRATCH)
    kv.extend_seq(SCRATCH, 1)
    for s, n in zip(SEQS, LENGTHS):
        kv.new_seq(s)
        kv.extend_seq(s, n + 1)  # room for the token the step appends
    return kv


def _state(kv, graph):
    from bee2bee_amd.engine.graphs import DecodeState

    runner = _DummyRunner()
    runner.kv = kv
    g = DecodeGraphs(runner, MAX_B, WIDTH) if graph else None
    return DecodeState(runner, g, SCRATCH)


def _rows(st):
    """The live rows, block tables at the width every backend has."""
    w = st.kv.block_table(st.seqs).shape[1]
    return [st.ids.tolist(), st.pos.tolist(), st.lens.tolist(),
            st.bt[:, :w].tolist()]


def test_decode_state_load_fills_live_and_pad_rows_only():
    kv = _kv()
    st = _state(kv, graph=True)
    g = st.graphs
    for buf in (g.input_ids, g.positions, g.seq_lens, g.block_table):
        buf.fill_(77)
    st.load(SEQS, LAST, LENGTHS)
    bt = kv.block_table(SEQS)
    assert g.bucket_for(3) == 4
    assert g.input_ids[:3].tolist() == LAST
    assert g.positions[:3].tolist() == LENGTHS
    assert g.seq_lens[:3].tolist() == [n + 1 for n in LENGTHS]
    assert torch.equal(g.block_table[:3, : bt.shape[1]], bt)
    # row 3 is the pad row of bucket 4: the scratch sequence, length 1
    sb = kv.block_table([SCRATCH])[0]
    assert g.input_ids[3] == 0 and g.positions[3] == 0 and g.seq_lens[3] == 1
    assert torch.equal(g.block_table[3, : sb.shape[0]], sb)
    # rows past the bucket are not this batch's to write
    for buf in (g.input_ids, g.positions, g.seq_lens, g.block_table):
        assert bool((buf[4:] == 77).all())


def test_decode_state_advance_bumps_in_place():
    kv = _kv()
    st = _state(kv, graph=True)
    g = st.graphs
    st.load(SEQS, LAST, LENGTHS)
    bufs = (g.input_ids, g.positions, g.seq_lens, g.block_table)
    ptrs = [b.data_ptr() for b in bufs]
    pad = [b[3].clone() for b in bufs]
    bt0 = g.block_table[:3].clone()

    for s, n in zip(SEQS, LENGTHS):
        kv.extend_seq(s, n + 2)  # no sequence reaches a new page yet
    nxt = torch.tensor([21, 22, 23])
    st.advance(nxt, False)
    assert g.input_ids[:3].tolist() == [21, 22, 23]
    assert g.positions[:3].tolist() == [n + 1 for n in LENGTHS]
    assert g.seq_lens[:3].tolist() == [n + 2 for n in LENGTHS]
    assert torch.equal(g.block_table[:3], bt0)

    # sequence 10 crosses a page boundary (length 4 -> 5), sequence 12
    # releases its first page
    for s, n in zip(SEQS, LENGTHS):
        kv.extend_seq(s, n + 3)
    assert kv.release_below(12, PAGE) == 1
    st.advance(torch.tensor([31, 32, 33]), True)
    bt = kv.block_table(SEQS)
    assert bt[0, 1] != 0 and bt[2, 0] == 0
    assert g.block_table[0, 1] == bt[0, 1] and bt0[0, 1] == 0
    assert g.block_table[2, 0] == 0 and bt0[2, 0] != 0
    assert torch.equal(g.block_table[:3, : bt.shape[1]], bt)
    assert g.positions[:3].tolist() == [n + 2 for n in LENGTHS]

    for b, p, row in zip(bufs, ptrs, pad):
        assert b.data_ptr() == p
        assert torch.equal(b[3], row)  # pad rows are written on load only


def test_decode_state_eager_holds_the_same_rows_with_a_narrow_table():
    kv = _kv()
    graph, eager = _state(kv, graph=True), _state(kv, graph=False)
    for st in (graph, eager):
        st.load(SEQS, LAST, LENGTHS)
    assert _rows(eager) == _rows(graph)
    assert eager.bt.shape == kv.block_table(SEQS).shape == (3, 3)
    assert eager.bt.is_contiguous()
    for s, n in zip(SEQS, LENGTHS):
        kv.extend_seq(s, n + 3)
    kv.release_below(12, PAGE)
    for st in (graph, eager):
        st.advance(torch.tensor([21, 22, 23]), True)
    assert _rows(eager) == _rows(graph)
    assert eager.bt.shape == kv.block_table(SEQS).shape


def test_decode_state_bump_equals_rebuild():
    nxt = [21, 22, 23]
    for graph in (True, False):
        kv = _kv()
        for s, n in zip(SEQS, LENGTHS):
            kv.extend_seq(s, n + 2)
        bumped, rebuilt = _state(kv, graph), _state(kv, graph)
        bumped.load(SEQS, LAST, LENGTHS)
        bumped.advance(torch.tensor(nxt), False)
        rebuilt.load(SEQS, nxt, [n + 1 for n in LENGTHS])
        assert _rows(bumped) == _rows(rebuilt)


def test_decode_state_bumps_only_with_ids_of_its_own_sequence_list():
    """The clobber: ids sampled for another batch (a prefill completion, a
    speculative subset) once became the decode inputs of this one."""
    for graph in (True, False):
        st = _state(_kv(), graph)
        ids = torch.tensor([21, 22, 23])
        assert st.pending(SEQS) is None  # never loaded: rebuild
        st.load(SEQS, LAST, LENGTHS)
        assert st.pending(SEQS) is None  # nothing sampled yet: rebuild
        st.hold(SEQS, ids)
        assert st.pending(SEQS) is ids
        assert st.pending(SEQS[:2]) is None  # membership changed: rebuild
        st.hold([11, 12, 13], torch.tensor([1, 2, 3]))
        assert st.pending(SEQS) is None  # another list's ids: rebuild
        st.hold(SEQS, ids)
        st.advance(st.pending(SEQS), False)
        assert st.pending(SEQS) is None  # consumed
        st.hold(SEQS, ids)
        st.forget()
        assert st.pending(SEQS) is None
