"""Cases of the sliding-window prefill attention (sqllm_attn_prefill_window_*): the case list only.  A case is tests/attn_append_cases'
expansion over six sequences built from one `seq_len`; the oracle and the gate are tests/attn_window_cases.reference_w.  Token t has
L = seq_len - (T - 1 - t) and attends [lo, L), lo = max(0, L - W); the kernel's tiles are 64 virtual rows x 64 keys.
  * ("paged", 17, ..., 40, 5)        W inside one key tile; a group of 3: 51 virtual rows, waves without rows.
  * ("bhsd", 17, ..., 90, 1)         W 1: every token attends its own key alone; L 74 .. 90, a tile starts behind tile 0.
  * ("paged", 33, ..., 120, 40)      group 1: lo of neighbouring tokens 48 .. 80, 63 / 64 / 65 inside one query tile.
  * ("padded", 64, ..., 124, 8)      group 1, W 8 behind 60 keys: the four waves of the tile have other tile ranges (wave 0 keys 53 .. 76,
                                     wave 3 keys 101 .. 124) and wave skips run; blocks of 5 straddle the tiles, strided heads and slots.
  * ("paged", 33, ..., 2P + 3, 20)   group 4: three query tiles, a tile edge inside a token, all tiles start far behind tile 0.
  * (..., 16, ..., 200, 64 / 65)     group 8, two full query tiles; W of exactly one key tile and one more.
  * (..., 82, 82), (..., 100, 2^31 - 1)  W at or above every L: the entry without a window, bit for bit.
  * sequences of a call              seq_len, seq_len, T (no prior context), seq_len, seq_len - 64 (another first tile), seq_len.
  * q_lens                           NULL, and the ragged classes of attn_append_cases.q_lens_for from class T: T, T + 1 (NaN rows),
                                     -3 (as 0), 0, 1, T - 1.
  * head_dim and dtype alternate; every geometry occurs.
"""
from tests import attn_append_cases as A
from tests import attn_decode_cases as C

P = C.P
INT32_MAX = (1 << 31) - 1
# (geometry, T, head_dim, query heads, kv heads, dtype, seq_len, W)
CASES = (
    ("paged", 17, 64, 6, 2, "fp16", 40, 5),
    ("bhsd", 17, 128, 2, 2, "bf16", 90, 1),
    ("paged", 33, 128, 2, 2, "fp16", 120, 40),
    ("padded", 64, 64, 2, 2, "bf16", 124, 8),
    ("paged", 33, 64, 8, 2, "bf16", 2 * P + 3, 20),
    ("paged", 16, 128, 16, 2, "fp16", 200, 64),
    ("padded", 16, 64, 16, 2, "bf16", 200, 65),
    ("paged", 17, 128, 6, 2, "bf16", 82, 82),
    ("bhsd", 33, 64, 8, 2, "fp16", 100, INT32_MAX),
)


def calls(T, seq_len):
    """((seq_lens, q_lens), ...): the six sequences of a case in one call, without q_lens and with the ragged classes"""
    seqs = (seq_len, seq_len, T, seq_len, max(seq_len - 64, 1), seq_len)
    return ((seqs, None), (seqs, A.q_lens_for(T, len(seqs), 3)))
