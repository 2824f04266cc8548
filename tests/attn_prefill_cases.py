"""Cases of the prefill attention (sqllm_attn_prefill): the case list only.  A case is tests/attn_append_cases' build / reference
at larger T; the oracle, the poisons and the gate are attn_decode_cases'.  The kernel's tiles are 64 virtual rows x 64 keys:
  * T x heads  1 (one row in a tile); 16 with a group of 8 (128 virtual rows: two full tiles); 17 (one past the append entries; with
               groups of 1 and 3: 17 and 51 rows, partial tiles and waves without rows); 33 with a group of 4 (132 virtual rows: a
               third tile, partial, a tile edge inside a token); 64 with a group of 1 (one token per row, a full tile) and of 8.
  * seq_lens   per call, one sequence each: T (no prior context), T - 3 (the first tokens have L <= 0; 0 for T = 1), T + 1,
               T + 63, T + 64, T + 65 (the last token's keys end one before, on and one behind a key-tile edge) and 2P + 3.
  * q_lens     NULL, and the ragged classes of attn_append_cases.q_lens_for: 0, 1, T - 1, T, T + 1 (NaN rows), -3 (as 0).
  * geometries paged; padded (blocks of 5 straddle key tiles, strided heads and slots); bhsd (one table entry per sequence).
  * head_dim and dtype alternate so that each occurs with each geometry and each group.
"""
from tests import attn_append_cases as A
from tests import attn_decode_cases as C

P = C.P
# (geometry, T, head_dim, query heads, kv heads, dtype)
CASES = (
    ("paged", 1, 64, 6, 2, "fp16"),
    ("padded", 16, 128, 16, 2, "bf16"),
    ("bhsd", 17, 64, 2, 2, "bf16"),
    ("paged", 17, 128, 6, 2, "fp16"),
    ("padded", 33, 64, 8, 2, "fp16"),
    ("paged", 33, 128, 8, 2, "bf16"),
    ("bhsd", 64, 128, 2, 2, "fp16"),
    ("padded", 64, 64, 2, 2, "bf16"),
    ("paged", 64, 64, 16, 2, "bf16"),
)


def seq_lens_for(T):
    return (T, max(T - 3, 0), T + 1, T + 63, T + 64, T + 65, 2 * P + 3)


def calls(T):
    """((seq_lens, q_lens), ...): the sequences of a T in one call, without q_lens and with the ragged classes"""
    seqs = seq_lens_for(T)
    return ((seqs, None), (seqs, A.q_lens_for(T, len(seqs), 3)))  # (from class T: the long sequences keep real tokens)
