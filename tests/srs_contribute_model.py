"""Shared by test_cpu_srs_contribute.py and test_gpu_srs_contribute.py: the scalars at which a signed fixed-window
multiplication (csrc/points_mul.hip) can go wrong."""
import random

from oracle import bls12_381 as ec

R = ec.R


def digits(window):
    return (256 + window - 1) // window


def edge_scalars(window):
    """For a signed window of `window` bits (digits -2^(w-1) .. 2^(w-1), 2^(w-1) the largest table index)."""
    half, full, ndig = 1 << (window - 1), 1 << window, digits(window)
    out = list(range(34))
    out += [R - 1, R - 2, (R - 1) // 2, (R + 1) // 2]
    for k in sorted(set(range(window, 255, window)) | {254}):
        out += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    # every digit the largest table index: +half in every window that keeps the scalar below r
    nd = ndig
    while sum(half << (window * j) for j in range(nd)) >= R:
        nd -= 1
    out.append(sum(half << (window * j) for j in range(nd)))
    # the recoding carries through every window: the lowest nibble half + 1 (negative digit, carry), every other one half
    # (half + carry: negative digit, carry), the top one the largest that stays below r; it takes the last carry
    top = (R >> (window * (ndig - 1))) - 1
    out.append((half + 1) + sum(half << (window * j) for j in range(1, ndig - 1)) + (top << (window * (ndig - 1))))
    out.append(((1 << 255) - 1) % R)
    # every unsigned digit full - 1: each window recodes to 0 or -1 under a carry
    out.append(sum((full - 1) << (window * j) for j in range(ndig - 1)))
    rnd = random.Random(0x51AB)
    out += [rnd.randrange(R) for _ in range(12)]
    assert all(0 <= k < R for k in out)
    return out


def carries_everywhere(k, window):
    """Whether the signed recoding of k carries out of every window below the top one."""
    half, c = 1 << (window - 1), 0
    for j in range(digits(window) - 1):
        v = ((k >> (window * j)) & ((1 << window) - 1)) + c
        c = 1 if v > half else 0
        if not c:
            return False
    return True


def all_largest_index(k, window):
    """Whether every window of k below its top bits holds 2^(w-1), the largest table index, with no carry anywhere."""
    half = 1 << (window - 1)
    return k.bit_length() > 248 and all(((k >> (window * j)) & ((1 << window) - 1)) == half for j in range(k.bit_length() // window))
