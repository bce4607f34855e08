"""Lane-level numpy model of mfcc_pair.hip's FFT data flow (index algebra check).

Emulates 64 lanes x 16 complex registers through pass 1, T1 (permlane32/16 swaps,
row_ror:8 exchange), pass 2, T2 (LDS combo layout), pass 3 and the pair split, and
checks the per-bin power of both frames against numpy.fft.rfft.

This file is the specification of the T2 layout (tests/test_pair_layout_cpu.py holds the kernel's
constants to it; tools/pair_lds_model.py prices its bank conflicts):
  * the T2 buffer is "b0-major": element b0 of a residue's 8-vector sits at complex index
    RS b0 + column, RS = row_stride(f64); reader lane L's slot A is column col(L), slot B col(L) + 64;
  * every lane runs the same 16 stores, instruction (h, c) storing register 8 h + c at
    base[store_reg(h, c)] + store_imm(h, c); store_bases() gives each lane's five bases.
Lanes with k1 & 7 == 0 (lanes 0-7) differ from the others only in the values of their bases."""
import numpy as np

L = np.arange(64)
PI = (0, 1, 2, 3, 4, 7, 6, 5)          # column order of the eight c0 of a k1 group
XI = (1, 2, 3, 0, 5, 6, 7, 4)          # the same for reader lanes 56..63 (residues of k1 = 0 and 8)
IRR = (56, 112, 40, 106, 114)          # the five store bases (columns) of the lanes with k1 & 7 == 0


def row_stride(f64=False):
    """complex per b0 row: = 2 mod 16 for the float32 ds_write_b64 groups, odd for float64's b128"""
    return 129 if f64 else 130


def q_of(a):
    return ((a & 1) ^ 1) + 16 * (a >> 1)


def col(lane):
    """column of reader lane `lane` (slot A; slot B is 64 further)"""
    a, c = lane >> 3, lane & 7
    return 2 * (PI[c] if a < 7 else XI[c]) + q_of(a)


def store_reg(h, c):
    return (1 if c >= 4 else 0) if h == 0 else (2 if c < 4 else 3 if c == 4 else 4)


def store_imm(h, c):
    """lane-uniform immediate (complex units) of store instruction (h, c)"""
    return 2 * PI[c] if h == 0 else 2 * PI[7 - c]


def store_bases(f64=False):
    """[lane][reg] -> complex index"""
    out = np.empty((64, 5), int)
    for lane in range(64):
        b0, kl = lane & 7, lane >> 3
        for i in range(5):
            u = IRR[i] if kl == 0 else (q_of(kl - 1) if i < 2 else 64 + q_of(7 - kl))
            out[lane, i] = row_stride(f64) * b0 + u
    return out


def residues():
    """(rA, rB) of the 64 reader lanes; lane 63 holds the self-paired residues 0 and 64"""
    rA = np.where(L < 56, (L >> 3) + 1 + 16 * (L & 7), np.where(L < 60, 8 + 16 * (L - 56), np.where(L < 63, 16 * (L - 59), 0)))
    return rA, np.where(L == 63, 64, 128 - rA)


def dft(x, axis):  # forward DFT along axis
    return np.fft.fft(x, axis=axis)


def model(x0, x1, f64=False):
    z = x0 + 1j * x1                       # windowing omitted (linear)
    v = np.empty((64, 16), complex)        # v[lane, reg]
    for a in range(16):
        v[:, a] = z[64 * a + L]
    v = dft(v, 1)                          # pass 1: DFT16 over a -> k1
    v *= np.exp(-2j * np.pi * np.outer(L, np.arange(16)) / 1024)
    # T1: reg bit2 <-> lane bit5 (permlane32_swap on (j, j+4))
    for j in range(16):
        if j & 4 == 0:
            a, b = v[:, j].copy(), v[:, j + 4].copy()
            v[:32, j], v[32:, j] = a[:32], b[:32]
            v[:32, j + 4], v[32:, j + 4] = a[32:], b[32:]
    for j in range(16):                    # reg bit1 <-> lane bit4 (permlane16_swap)
        if j & 2 == 0:
            a, b = v[:, j].copy(), v[:, j + 2].copy()
            na, nb = a.copy(), b.copy()
            for r in range(4):
                s = slice(16 * r, 16 * r + 16)
                if r % 2 == 0:
                    na[s] = a[s]; nb[s] = a[16 * (r + 1):16 * (r + 2)]
                else:
                    na[s] = b[16 * (r - 1):16 * r]; nb[s] = b[s]
            v[:, j], v[:, j + 2] = na, nb
    hi3 = (L & 8) != 0
    for j in range(0, 16, 2):              # reg bit0 <-> lane bit3 (row_ror:8 = lane ^ 8)
        a, b = v[:, j].copy(), v[:, j + 1].copy()
        v[:, j] = np.where(hi3, b[L ^ 8], a)
        v[:, j + 1] = np.where(hi3, b, a[L ^ 8])
    b0 = L & 7
    for h in range(2):                     # pass 2: DFT8 over b1 -> c0, twiddle w64^{b0 c0}
        v[:, 8 * h:8 * h + 8] = dft(v[:, 8 * h:8 * h + 8], 1)
        v[:, 8 * h:8 * h + 8] *= np.exp(-2j * np.pi * np.outer(b0, np.arange(8)) / 64)
    # T2 through a flat LDS image (complex units): 16 stores, the same for every lane
    RS = row_stride(f64)
    lds = np.full(8 * RS, np.nan, complex)
    base = store_bases(f64)
    for h in range(2):
        for c in range(8):
            addr = base[:, store_reg(h, c)] + store_imm(h, c)
            assert np.isnan(lds[addr]).all() and len(set(addr)) == 64
            lds[addr] = v[:, 8 * h + c]
    assert np.isnan(lds).sum() == 8 * (RS - 128)
    cl = np.array([col(lane) for lane in range(64)])
    v = np.stack([np.concatenate([lds[cl[lane] + RS * np.arange(8)], lds[cl[lane] + 64 + RS * np.arange(8)]])
                  for lane in range(64)])
    v[:, :8] = dft(v[:, :8], 1)           # pass 3
    v[:, 8:] = dft(v[:, 8:], 1)
    rA, rB = residues()
    P0 = np.full(513, np.nan); P1 = np.full(513, np.nan)

    def pw(a, b, k):
        s = a + np.conj(b); d = a - np.conj(b)
        assert np.isnan(P0[k]), k
        P0[k] = abs(s) ** 2 / 4; P1[k] = abs(d) ** 2 / 4

    for lane in range(64):
        self = lane == 63
        A, B = v[lane, :8], v[lane, 8:]
        for c in range(4):
            pw(A[c], A[(8 - c) & 7] if self else B[7 - c], rA[lane] + 128 * c)
        pw(B[4] if self else A[4], B[3], rB[lane] + 384)
        for c in range(5, 8):
            pw(B[c] if self else A[c], B[7 - c], rB[lane] + 128 * (7 - c))
        if self:
            pw(A[4], A[4], 512)
    return P0, P1


def main():
    rng = np.random.default_rng(0)
    x0, x1 = rng.standard_normal(1024), rng.standard_normal(1024)
    for f64 in (False, True):
        P0, P1 = model(x0, x1, f64)
        R0, R1 = abs(np.fft.rfft(x0)) ** 2, abs(np.fft.rfft(x1)) ** 2
        print("max rel err frame t  :", np.max(abs(P0 - R0) / R0.max()))
        print("max rel err frame t+1:", np.max(abs(P1 - R1) / R1.max()))
        assert np.allclose(P0, R0, rtol=1e-9, atol=1e-9 * R0.max()) and np.allclose(P1, R1, rtol=1e-9, atol=1e-9 * R1.max())
    print("pair model OK")


if __name__ == "__main__":
    main()
