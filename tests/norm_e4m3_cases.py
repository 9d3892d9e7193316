"""Case table of yume_adaln_modulate_e4m3 (tests/test_norm_e4m3_gpu.py, tests/test_norm_e4m3_cabi.py).

The call is DEFINED as yume_quant_rows_e4m3 applied to what yume_adaln_modulate(..., out_kind = 0) stores, so the yardstick is that two-call
composite on the same device inputs, bit for bit: q bytes and fp32 scales. Shapes: T in {1, 5, 1027} (1027 >= 1024 reaches the two-row
instance at C <= 3072, with an odd tail row), C in {512, 3072, 5120} (adaln<3> / adaln2, adaln<3> / adaln2, adaln<5>) plus one C = 8192 row
for adaln<8>; with and without row_idx; add_one both ways; ldq = C + 16 with guard bytes, one guard row behind T.

The exactly-zero row: x constant over the row (a power of two, so the mean is exact and x - mean = 0) and a modulation row whose `add` is 0.
With row_idx the row points at such a modulation row (row ZERO_MOD of the table); without row_idx every token shares modulation row 0, so
the separate `zero_add` rows use an all-zero `add`.
"""
import torch

GUARD_BYTE = 0xA5
GUARD_SCALE = -7.0
N_MOD = 4            # modulation rows of the table
ZERO_MOD = 3         # the one whose `add` is zero

# (name, T, C, row_idx, add_one, zero_add)
CASES = []
for T in (1, 5, 1027):
    for C in (512, 3072, 5120):
        for use_idx in (False, True):
            for add_one in (True, False):
                CASES.append((f"T{T}_C{C}_{'idx' if use_idx else 'noidx'}_{'one' if add_one else 'raw'}", T, C, use_idx, add_one, False))
CASES.append(("T5_C512_noidx_zero_row", 5, 512, False, True, True))
CASES.append(("T1027_C3072_noidx_zero_row", 1027, 3072, False, True, True))
CASES.append(("T5_C8192_idx_one", 5, 8192, True, True, False))
IDS = [c[0] for c in CASES]

# the log name of the instance a case must run on (YUME_NORM_LOG=1)
def instance(T, C):
    if C <= 3072 and T >= 1024:
        return "adaln2_e4m3"
    return "adaln_e4m3<%d>" % (3 if C <= 3072 else 5 if C <= 5120 else 8)


def zero_row_of(T):
    return min(3, T - 1)


def make_case(T, C, use_idx, add_one, zero_add, seed=0):
    """host tensors: x fp32 [T, C + 4] (ldx > C), table fp32 [N_MOD, 2, C] (mul = table[:, 0], add = table[:, 1], tab_stride = 2 C),
    row_idx int32 [T] or None"""
    g = torch.Generator().manual_seed(1000 * T + C + seed)
    x = torch.randn(T, C + 4, generator=g) * 3.0 + 0.5
    x[:, ::97] *= 8.0                                              # a few outliers per row: the amax is not a typical element
    tab = torch.randn(N_MOD, 2, C, generator=g) * 0.5
    tab[ZERO_MOD, 1] = 0.0
    if zero_add:
        tab[:, 1] = 0.0
    idx = None
    if use_idx:
        # runs of equal rows (tokens of one timestep are contiguous) with the changes at odd AND even positions: the two rows of an adaln2
        # workgroup carry one modulation row or two
        idx = ((torch.arange(T) + 1) // 3 % (N_MOD - 1)).to(torch.int32)
    if use_idx or zero_add:
        z = zero_row_of(T)
        x[z] = 2.0
        if use_idx:
            idx[z] = ZERO_MOD
    return x, tab, idx
