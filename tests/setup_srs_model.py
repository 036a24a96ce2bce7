"""Big-integer model of a phase-1 transcript and of the transform of point arrays (zkmi_srs_*, zkmi_g{1,2}_points_ntt_dev)
over the oracle's point arithmetic: the shared inputs of tests/test_{cpu,gpu}_setup_srs.py.  The transform is the O(N^2)
definition, one scalar multiplication per term."""
from oracle import bls12_381 as ec
from oracle import ntt as nt

R = ec.R
FIELD = {1: ec.Fq, 2: ec.Fq2}
TO_BYTES = {1: ec.g1_to_bytes, 2: ec.g2_to_bytes}
FROM_BYTES = {1: ec.g1_from_bytes, 2: ec.g2_from_bytes}
WIRE = {1: 96, 2: 192}


def frs(vals):
    return b"".join(ec.fr_to_bytes(v) for v in vals)


def points_bytes(group, pts):
    return b"".join(TO_BYTES[group](p) for p in pts)


def points_from_bytes(group, b):
    w = WIRE[group]
    return [FROM_BYTES[group](b[w * i : w * i + w]) for i in range(len(b) // w)]


def transcript(tau, alpha, beta, log_n, extra=0):
    """The five sections for a domain of 2^log_n (`extra` more powers in every array): what zkmi_srs_generate makes."""
    n = 1 << log_n
    pw = [pow(tau, i, R) for i in range(2 * n - 1 + extra)]
    return {
        "tau_g1": [ec.g1_mul(p) for p in pw],
        "tau_g2": [ec.g2_mul(p) for p in pw[: n + extra]],
        "alpha_tau_g1": [ec.g1_mul(alpha * p) for p in pw[: n + extra]],
        "beta_tau_g1": [ec.g1_mul(beta * p) for p in pw[: n + extra]],
        "beta_g2": ec.g2_mul(beta),
    }


def dft_points(group, pts, inverse=False):
    """out[i] = sum_k w^(ik) pts[k], inverse: N^-1 sum_k w^(-ik) pts[k] -- the definition, N^2 scalar multiplications."""
    F, n = FIELD[group], len(pts)
    log_n = n.bit_length() - 1
    assert 1 << log_n == n
    w = nt.root_of_unity(log_n) if log_n else 1
    if inverse:
        w = pow(w, R - 2, R)
    scale = pow(n, R - 2, R) if inverse else 1
    out = []
    for i in range(n):
        acc = None
        for k, p in enumerate(pts):
            acc = ec.pt_add(F, acc, ec.pt_mul(F, p, pow(w, i * k, R) * scale % R))
        out.append(acc)
    return out
