"""The Verify arm's host side, no GPU: vdb_g2_mul_generator and vdb_pairing_check (halo2_vectordb_amd/csrc/pairing.cpp) against the
Python pairing of oracle/pairing.py, and the protocol of halo2_vectordb_amd/verifier.py on a proof of the oracle's CPU prover
(BASELINE C1), with the two device stages — decompression and the MSM — done by the oracle instead."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def _fq_limbs(v):
    from oracle import pairing as PR
    m = (v << 256) % PR.Q
    return [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def g1(p):
    return np.zeros(8, dtype=np.uint64) if p is None else np.array(_fq_limbs(p[0]) + _fq_limbs(p[1]), dtype=np.uint64)


def g2(p):
    if p is None:
        return np.zeros(16, dtype=np.uint64)
    return np.array(_fq_limbs(p[0].c[0]) + _fq_limbs(p[0].c[1]) + _fq_limbs(p[1].c[0]) + _fq_limbs(p[1].c[1]), dtype=np.uint64)


def check(pairs):
    from halo2_vectordb_amd import verifier
    a = np.stack([g1(p) for p, _ in pairs]) if pairs else np.zeros((0, 8), dtype=np.uint64)
    b = np.stack([g2(q) for _, q in pairs]) if pairs else np.zeros((0, 16), dtype=np.uint64)
    return verifier.pairing_check(a, b)


@pytest.mark.parametrize("s", ["random0", "random1", 0, 1, "r-1"])
def test_g2_mul_generator_is_the_oracles(s):
    from halo2_vectordb_amd import verifier
    from oracle import pairing as PR
    s = {"r-1": PR.R - 1}.get(s, s)
    if isinstance(s, str):
        s = random.Random(s).randrange(PR.R)
    assert np.array_equal(verifier._g2_generator_times(s), g2(PR.pt_mul(PR.G2, s)))


def test_pairing_product_accepts_bilinearity_and_rejects_an_off_by_one():
    from oracle import pairing as PR
    rng = random.Random(7)
    a, b = rng.randrange(1, PR.R), rng.randrange(1, PR.R)
    P, Q = PR.pt_mul(PR.G1, rng.randrange(1, PR.R)), PR.pt_mul(PR.G2, rng.randrange(1, PR.R))
    assert check([(PR.pt_mul(P, a), PR.pt_mul(Q, b)), (PR.pt_neg(PR.pt_mul(P, a * b % PR.R)), Q)])
    assert not check([(PR.pt_mul(P, a), PR.pt_mul(Q, b + 1)), (PR.pt_neg(PR.pt_mul(P, a * b % PR.R)), Q)])
    assert not check([(PR.pt_mul(P, a + 1), PR.pt_mul(Q, b)), (PR.pt_neg(PR.pt_mul(P, a * b % PR.R)), Q)])
    # the oracle agrees on both
    assert PR.pairing_product_is_one([(PR.pt_mul(P, a), PR.pt_mul(Q, b)), (PR.pt_neg(PR.pt_mul(P, a * b % PR.R)), Q)])


def test_pairing_with_the_identity_in_either_slot_and_any_number_of_pairs():
    from oracle import pairing as PR
    P, Q = PR.pt_mul(PR.G1, 5), PR.pt_mul(PR.G2, 11)
    assert check([])                                           # n = 0: the empty product
    assert check([(None, Q)]) and check([(P, None)]) and check([(None, None)])
    assert not check([(P, Q)])                                 # n = 1: e is non-degenerate
    # n = 3: e(2P, Q) e(3P, Q) e(-5P, Q) = 1, with an identity pair beside it too
    assert check([(PR.pt_mul(P, 2), Q), (PR.pt_mul(P, 3), Q), (PR.pt_neg(PR.pt_mul(P, 5)), Q)])
    assert check([(PR.pt_mul(P, 2), Q), (None, Q), (PR.pt_neg(PR.pt_mul(P, 2)), Q)])
    assert not check([(PR.pt_mul(P, 2), Q), (PR.pt_mul(P, 3), Q), (PR.pt_neg(PR.pt_mul(P, 4)), Q)])


def test_points_off_their_curves_are_an_argument_error():
    from halo2_vectordb_amd import _lib
    from oracle import pairing as PR
    L = _lib.load()
    P, Q = g1(PR.G1), g2(PR.G2)
    ok = ctypes.c_int(7)
    bad_p = P.copy()
    bad_p[4:] = _fq_limbs(3)
    bad_q = Q.copy()
    bad_q[8:12] = _fq_limbs(5)
    for a, b in ((bad_p, Q), (P, bad_q)):
        rc = L.vdb_pairing_check(a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1), ctypes.byref(ok))
        assert rc == -3 and ok.value == 7


def _oracle_stages(monkeypatch, O):
    """the verifier's two device stages done by the oracle (test only: the product has no such fallback)"""
    from halo2_vectordb_amd import verifier
    from test_gpu_rounds import _decompress

    def decompress(enc, sign_bit=6):
        enc = bytes(enc)
        pts, st = [], []
        for i in range(len(enc) // 32):
            try:
                pts.append(_decompress(O, enc[32 * i: 32 * i + 32]))
                st.append(0)
            except AssertionError:
                pts.append(np.zeros(8, dtype=np.uint64))
                st.append(2)
        return np.stack(pts), np.array(st, dtype=np.uint8)
    monkeypatch.setattr(verifier, "decompress", decompress)
    monkeypatch.setattr(verifier, "msm_points", lambda pts, sc: O.msm_naive(np.asarray(sc), np.asarray(pts)).reshape(8))


def test_the_verifier_protocol_on_a_cpu_proof(monkeypatch, O):
    """C1 proved by the oracle's CPU prover: verifier.verify accepts it and rejects a flipped byte, another statement, a short and a
    long proof, a missing public value, and a key that states another constraint degree.  The protocol's opening table is what the
    prover opened, and a key without that record (which falls back to the table) accepts and rejects the same"""
    from halo2_vectordb_amd import protocol, verifier
    from oracle import prover as PV
    import test_oracle_prover_cpu as C1
    _oracle_stages(monkeypatch, O)
    cs, pk, out, _stream, _lookup, _dist = C1._prove(O, PV)
    meta = dict(rows=cs.rows, k=cs.k, n_adv=cs.n_adv, n_lk=cs.n_lk, n_cols=cs.n_cols, n_sets=cs.n_sets, chunk_len=cs.chunk_len, n_blind=PV.N_BLIND,
                delta=O.DELTA_INT, n_instances=len(cs.instance_cells))
    vk = verifier.VerifyingKey(meta, {name: pk.commits[name] for name in verifier.FIXED}, out["opened"], tau=C1.TAU)
    proof, inst = out["proof"], out["instances"]
    timings = {}
    assert verifier.verify(proof, inst, vk, timings=timings)
    assert set(timings) == {"decompress", "transcript", "algebra", "msm", "pairing"}
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 1
    assert not verifier.verify(bytes(bad), inst, vk)
    assert not verifier.verify(proof, [(inst[0] + 1) % O.R_MOD], vk)
    assert not verifier.verify(proof, [inst[0] + O.R_MOD], vk)              # a public value that is not below r
    assert not verifier.verify(proof[:-32], inst, vk) and not verifier.verify(proof + bytes(32), inst, vk)
    assert not verifier.verify(proof, [], vk)
    wrong = verifier.VerifyingKey({**meta, "chunk_len": 1}, vk.fixed, out["opened"], tau_g2=vk.tau_g2)
    assert not verifier.verify(proof, inst, wrong)
    assert not verifier.verify(proof, inst, verifier.VerifyingKey(meta, vk.fixed, out["opened"], tau=C1.TAU + 1))
    assert protocol.opened(cs.n_lk, protocol.N_BLIND) == out["opened"]
    default = verifier.VerifyingKey(meta, vk.fixed, None, tau=C1.TAU)
    assert default.opened == out["opened"]
    assert verifier.verify(proof, inst, default) and not verifier.verify(bytes(bad), inst, default)
