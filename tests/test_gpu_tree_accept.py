"""sqllm_tree_accept and sqllm_kv_compact on the GPU (quant.tree_accept / quant.compact_kv, route="kernel") against the loop
references of tests/tree_accept_cases.py: integers and bytes, compared exactly -- the caches as WHOLE buffers, guards included."""
import numpy as np
import pytest
import torch

from tests import tree_accept_cases as TA
from tests.test_tree_accept_cpu import _signed

gpu_test = pytest.mark.gpu
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn}
T, H, KEYS, GUARD = 64, 2, 320, 64  # nodes, kv heads, keys per table row, guard elements on both sides of a cache


def _accept_operands(gpu, tree, T):
    par, words, draft, target, q_lens = lists = TA.accept_batch(tree, T)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=gpu)  # noqa: E731
    return lists, (i32(par), torch.tensor(_signed(words), dtype=torch.int64, device=gpu), i32(draft), i32(target), i32(q_lens))


@gpu_test
@pytest.mark.parametrize("tree", TA.TREES)
@pytest.mark.parametrize("T", TA.SIZES)
def test_tree_accept_is_the_loop_reference(gpu, tree, T):
    import ctypes

    from squeezellm_amd import _lib
    from squeezellm_amd.quant import tree_accept

    lists, ops = _accept_operands(gpu, tree, T)
    seq = [300 + b for b in range(len(lists[0]))]
    want = TA.accept_ref(*lists, T, seq)
    sl = torch.tensor(seq, dtype=torch.int32, device=gpu)
    got = tree_accept(*ops, seq_lens=sl, route="kernel")
    assert [g.tolist() for g in got] == list(want) and sl.tolist() == seq  # (seq_lens_out separate: the input stays)
    # ... and seq_lens_out aliased to seq_lens_in, through the C entry
    a = _lib.SqllmTreeAccept()
    outs = [torch.full(s, 77, dtype=torch.int32, device=gpu) for s in ((len(seq),), (len(seq), T), (len(seq),))]
    a.parents, a.tree_mask, a.draft_tokens, a.target_tokens, a.q_lens = (o.data_ptr() for o in ops)
    a.accept_len, a.path, a.next_token = (o.data_ptr() for o in outs)
    a.seq_lens_in = a.seq_lens_out = sl.data_ptr()
    a.stride, a.mask_stride, a.q_len, a.batch = T, 2 * T, T, len(seq)
    assert _lib.load().sqllm_tree_accept(ctypes.byref(a), torch.cuda.current_stream(gpu).cuda_stream) == 0
    assert [o.tolist() for o in outs] + [sl.tolist()] == list(want)


class Caches:
    """n caches of one geometry inside guarded element buffers, every element a function of (cache, index): all 16-bit patterns occur,
    NaN and inf among them"""

    def __init__(self, gpu, kind, D, dtype_name, n_caches, B, odd=False):
        self.dtype, self.D = DTYPES[dtype_name], D
        self.geo = self.bs, self.table, self.n_slots, self.ss, self.hs = TA.geometry(kind, B, H, D, KEYS)
        self.base = GUARD + (1 if odd else 0)
        n = self.base + (self.n_slots - 1) * self.ss + (H - 1) * self.hs + D + GUARD
        self.bufs = [torch.from_numpy(TA.pattern(n, c, 1 if dtype_name == "fp8" else 2)).to(gpu) for c in range(n_caches)]
        self.views = [b.view(self.dtype).as_strided((self.n_slots, H, D), (self.ss, self.hs, 1), self.base) for b in self.bufs]

    def numpy(self):
        return [b.cpu().numpy().copy() for b in self.bufs]


def _compact(gpu, c, table, seq, q_lens, path, alen):
    from squeezellm_amd.quant import compact_kv

    i32 = lambda x: torch.tensor(np.asarray(x), dtype=torch.int32, device=gpu)  # noqa: E731
    compact_kv(c.views, i32(table), i32(seq), T, i32(path), i32(alen), block_size=c.bs, q_lens=i32(q_lens), route="kernel")
    torch.cuda.synchronize()


COMPACT = [("paged", 128, "bf16", 6, False), ("paged", 64, "fp16", 1, False), ("padded", 128, "fp16", 1, False), ("padded", 64, "bf16", 6, False),
           ("pad4", 128, "bf16", 1, False), ("bhsd", 128, "fp16", 1, False), ("bhsd", 64, "fp8", 6, False), ("paged", 128, "fp8", 6, False),
           ("paged", 64, "fp8", 1, False), ("padded", 128, "fp8", 1, True), ("padded", 64, "fp8", 6, True), ("pad4", 64, "fp8", 1, False)]


@gpu_test
@pytest.mark.parametrize("kind,D,dtype_name,n_caches,odd", COMPACT)
def test_compact_kv_is_the_loop_reference_on_the_whole_buffers(gpu, kind, D, dtype_name, n_caches, odd):
    ctx, q_lens, alen, path = TA.compact_batch(T)
    seq = [c + n for c, n in zip(ctx, q_lens)]
    c = Caches(gpu, kind, D, dtype_name, n_caches, len(seq), odd)
    table = c.table.copy()
    if kind != "bhsd":  # one source row's table entry leads outside the cache: that element is skipped, nothing there is read
        table[TA.BAD_KEY[0], TA.BAD_KEY[1] // c.bs] = 1 << 20
    geo = (c.bs, table, c.n_slots, c.ss, c.hs)
    before = c.numpy()
    want = [b.copy() for b in before]
    TA.compact_ref(want, c.base, geo, H, D, seq, q_lens, T, path, alen)
    _compact(gpu, c, table, seq, q_lens, path, alen)
    got = c.numpy()
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert not any(np.array_equal(g, b) for g, b in zip(got, before))  # every cache moved
    # a sequence alone leaves the same bytes in its own rows (the shift chain: sequence 0)
    alone = Caches(gpu, kind, D, dtype_name, n_caches, len(seq), odd)
    _compact(gpu, alone, table[:1], seq[:1], q_lens[:1], path[:1], alen[:1])
    rows = [table[0, p // c.bs] * c.bs + p % c.bs for p in range(ctx[0], seq[0])]
    for g, a in zip(got, alone.numpy()):
        for s in rows:
            for h in range(H):
                at = c.base + s * c.ss + h * c.hs
                assert np.array_equal(g[at:at + D], a[at:at + D])


@gpu_test
def test_both_calls_in_one_captured_graph_follow_operands_updated_in_place(gpu):
    from squeezellm_amd.quant import compact_kv, tree_accept

    lists, ops = _accept_operands(gpu, "heap", T)
    B = len(lists[0])
    c = Caches(gpu, "paged", 128, "bf16", 4, B)
    seq = torch.tensor([T + 14] * B, dtype=torch.int32, device=gpu)
    table = torch.tensor(c.table, dtype=torch.int32, device=gpu)
    out = []

    def run():
        out[:] = tree_accept(*ops, seq_lens=seq, route="kernel")
        compact_kv(c.views, table, seq, T, out[1], out[0], block_size=c.bs, q_lens=ops[4], route="kernel")

    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    fresh = c.numpy()
    for step, ctx in enumerate((0, 255, 30)):  # in place: the graph holds the addresses
        par, words, draft, target, q_lens = lists
        draft = [row[step:] + row[:step] for row in draft] if step else draft  # other tokens: other paths
        ops[2].copy_(torch.tensor(draft, dtype=torch.int32))
        seq.fill_(T + ctx)
        for buf, f in zip(c.bufs, fresh):
            buf.copy_(torch.from_numpy(f))
        g.replay()
        torch.cuda.synchronize()
        seqs = [T + ctx] * B
        alen, path, nxt, new_seq = TA.accept_ref(par, words, draft, target, q_lens, T, seqs)
        assert [o.tolist() for o in out] == [alen, path, nxt, new_seq], step
        want = [f.copy() for f in fresh]
        TA.compact_ref(want, c.base, c.geo, H, 128, seqs, q_lens, T, np.asarray(path), alen)
        assert all(np.array_equal(g_, w) for g_, w in zip(c.numpy(), want)), step
