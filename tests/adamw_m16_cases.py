"""The bf16-moment AdamW step (mla_adamw_m16_step, include/mla_hip_optim.h) in numpy: Philox4x32-10, the element -> random word
mapping, stochastic rounding to bf16 and the step itself -- shared by tests/test_adamw_m16_cases_host.py, test_adamw_m16_gpu.py and the
host LocalOps of test_fsdp_m16_gloo.py.

The arithmetic of the step is trunk_cases.adamw_emul32's (adamw_elem of elementwise.hip, every contraction as written there), called on
the moments decoded from bf16; the new master comes from the UNROUNDED fp32 moments, which are then stored as
  m16' = sr16(m', r & 0xffff), v16' = sr16(v', r >> 16),
r = word (e & 3) of Philox4x32-10(counter (lo32(e >> 2), hi32(e >> 2), step, 0), key (lo32(seed), hi32(seed))) for the element with
global index e = index_base + i."""
import numpy as np
import torch

import trunk_cases as T

PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
# (counter, key) -> output: the known answers of the Random123 distribution for Philox4x32-10
PHILOX_KAT = (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
              ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)))
SEED = 0x1234ABCD5678EF01          # both key words non-zero and different
INDEX_BASES = (0, 8, 3, 2 ** 34 + 4)
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two. Returns the four output words as uint32 arrays."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _M32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k = [np.uint64(int(x) & 0xFFFFFFFF) for x in key]
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M[0]) * c[0], np.uint64(PHILOX_M[1]) * c[2]          # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> sh) ^ c[1] ^ k[0], p1 & _M32, (p0 >> sh) ^ c[3] ^ k[1], p0 & _M32]
        k = [(k[0] + np.uint64(PHILOX_W[0])) & _M32, (k[1] + np.uint64(PHILOX_W[1])) & _M32]
    return [x.astype(np.uint32) for x in c]


def element_counter(e, step):
    """(counter, word) of the element with global index e: ((lo32(e >> 2), hi32(e >> 2), uint32(step), 0), e & 3)."""
    e4 = int(e) >> 2
    return (e4 & 0xFFFFFFFF, e4 >> 32, int(step) & 0xFFFFFFFF, 0), int(e) & 3


def random_words(n, seed, step, index_base):
    """uint32 [n]: r of the elements index_base .. index_base + n - 1 (one Philox call per group of four global indices)."""
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    e = np.arange(n, dtype=np.int64) + np.int64(index_base)
    g0, g1 = int(e[0]) >> 2, int(e[-1]) >> 2
    g = np.arange(g0, g1 + 1, dtype=np.int64).astype(np.uint64)
    words = np.stack(philox4x32_10((g & _M32, g >> np.uint64(32), int(step) & 0xFFFFFFFF, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)), axis=1)
    return words[(e >> 2) - g0, e & 3]


def bf16_bits(t):
    """torch bf16 tensor -> numpy uint16 bit patterns."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(b):
    """numpy uint16 bit patterns -> torch bf16 tensor."""
    return torch.from_numpy(np.ascontiguousarray(b, dtype=np.uint16).view(np.int16).copy()).view(torch.bfloat16)


def decode(b):
    """bf16 bit patterns -> fp32 values (numpy): float(bits << 16)."""
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def rne16(x):
    """fp32 -> bf16 bits, round-to-nearest-even (torch's cast; f2bf of the kernels)."""
    return bf16_bits(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16))


def sr16(x, r16):
    """fp32 -> bf16 bits, stochastically rounded with the 16 random bits r16: (bits(x) + r16) >> 16 for finite x (a carry into the
    exponent is the correct round-up), round-to-nearest-even for inf / NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    out = ((b + (np.asarray(r16, dtype=np.uint64) & np.uint64(0xFFFF))) >> np.uint64(16)).astype(np.uint16)
    special = (b & np.uint64(0x7F800000)) == np.uint64(0x7F800000)
    return np.where(special, rne16(x), out)


def adamw_m16_emul32(p, g, m16, v16, step, wd, gs, n_decay=None, seed=0, index_base=0, rounding="sr", **hyper):
    """One step. p, g: fp32 torch tensors; m16, v16: bf16 torch tensors; elements [0, n_decay) are weight-decayed (None: all).
    rounding = "rne" stores the moments round-to-nearest instead (the scheme that does not work).
    Returns (p', m16', v16', m', v'): the new master, the stored moments (bf16 tensors) and the unrounded fp32 moments."""
    n = p.numel()
    n_decay = n if n_decay is None else n_decay
    m, v = torch.from_numpy(decode(bf16_bits(m16))), torch.from_numpy(decode(bf16_bits(v16)))
    pc, gc = p.detach().cpu(), g.detach().cpu()
    pp, mm, vv = T.adamw_emul32(pc, gc, m, v, step, wd, gs, **hyper)
    if n_decay < n:        # the not-decayed group: the same arithmetic with decay = 1
        pp = torch.cat([pp[:n_decay], T.adamw_emul32(pc[n_decay:], gc[n_decay:], m[n_decay:], v[n_decay:], step, 0.0, gs, **hyper)[0]])
    if rounding == "rne":
        m_out, v_out = rne16(mm.numpy()), rne16(vv.numpy())
    else:
        r = random_words(n, seed, step, index_base)
        m_out, v_out = sr16(mm.numpy(), r & np.uint32(0xFFFF)), sr16(vv.numpy(), r >> np.uint32(16))
    return pp, from_bits(m_out), from_bits(v_out), mm, vv


def m16_state(family, n, tag=0):
    """trunk_cases.adamw_state with the moments as bf16 tensors (rounded to nearest): (p, g, m16, v16)."""
    p, g, m, v = T.adamw_state(family, n, tag)
    return p, g, m.to(torch.bfloat16), v.to(torch.bfloat16)


def ulp16_of(x):
    """Spacing of bf16 at the fp32 values x (numpy fp64): 2^(exponent - 7), the subnormal spacing 2^-133 below 2^-126."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    ex = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (ex - 7)
