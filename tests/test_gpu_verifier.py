"""The Verify arm on the device (halo2_vectordb_amd/verifier.py; include/vdb.h b7): vdb_g1_decompress_dev against the test verifier's
_decompress and the oracle, vdb_msm_points_dev against oracle.msm_naive / oracle.msm, and verifier.verify against the test verifier
(_verify of tests/test_gpu_rounds.py) on the proofs of the cosine k-means, Merkle and query circuits — accepted, and rejected for
every tampering the yardstick rejects — then through the proof and key files, the command line, and C4' at full size."""
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest

from test_gpu_rounds import FIXED, Q_MOD, TAU, _decompress, _meta, _verify

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _random_points(rng, n):
    """n random affine points (integers) by rejection on x: y = (x^3 + 3)^((q+1)/4) when it is a root, either sign"""
    out = []
    while len(out) < n:
        x = int.from_bytes(rng.bytes(32), "little") % Q_MOD
        rhs = (x * x * x + 3) % Q_MOD
        y = pow(rhs, (Q_MOD + 1) // 4, Q_MOD)
        if y * y % Q_MOD == rhs:
            out.append((x, y if rng.integers(2) else Q_MOD - y))
    return out


def _encode(x, y, sign_bit):
    return (x | ((y & 1) << (248 + sign_bit))).to_bytes(32, "little")


def _points_array(O, pts):
    return O.fq_from_ints([v for p in pts for v in p]).reshape(-1, 8) if pts else np.zeros((0, 8), dtype=np.uint64)


@pytest.mark.parametrize("sign_bit", [6, 7])
def test_decompression_is_bit_equal_to_the_test_verifiers(api, O, sign_bit):
    from halo2_vectordb_amd import verifier
    rng = np.random.default_rng(sign_bit)
    pts = _random_points(rng, 10_000)
    enc = b"".join(_encode(x, y, sign_bit) for x, y in pts)
    got, status = verifier.decompress(enc, sign_bit)
    assert not status.any()
    assert np.array_equal(got, _points_array(O, pts))
    if sign_bit == 6:                                     # the yardstick's own decoder reads bit 6
        for i in range(0, 10_000, 97):
            assert np.array_equal(got[i], _decompress(O, enc[32 * i: 32 * i + 32]))


@pytest.mark.parametrize("sign_bit", [6, 7])
def test_decompression_status_of_malformed_encodings(api, O, sign_bit):
    from halo2_vectordb_amd import verifier
    rng = np.random.default_rng(40 + sign_bit)
    (x, y), = _random_points(rng, 1)
    other = 13 - sign_bit                                 # the spare top bit that is not the sign
    no_root = next(v for v in range(1, 100) if pow((v ** 3 + 3) % Q_MOD, (Q_MOD - 1) // 2, Q_MOD) != 1)
    cases = [
        (bytes(32), 0),                                                   # the identity
        (_encode(x, y, sign_bit), 0),
        ((Q_MOD).to_bytes(32, "little"), 1),                              # x = q
        ((Q_MOD + 5).to_bytes(32, "little"), 1),                          # x >= q
        ((x | (1 << (248 + other))).to_bytes(32, "little"), 1),          # the other spare bit set
        (no_root.to_bytes(32, "little"), 2),                              # x^3 + 3 is not a square
        ((1 << (248 + sign_bit)).to_bytes(32, "little"), 3),             # the identity with the sign flag
        ((1 << (248 + other)).to_bytes(32, "little"), 3),                # ... with the other flag
        ((3 << 254).to_bytes(32, "little"), 3),                           # ... with both
    ]
    got, status = verifier.decompress(b"".join(e for e, _ in cases), sign_bit)
    assert list(status) == [s for _, s in cases]
    assert not got[[i for i, (_, s) in enumerate(cases) if s]].any()     # rejected points come out as (0, 0)
    assert not got[0].any() and np.array_equal(got[1], _points_array(O, [(x, y)])[0])
    if sign_bit == 6:
        assert np.array_equal(got[1], _decompress(O, cases[1][0]))


def _msm_want(O, scalars, bases):
    if len(bases) == 0:
        return np.zeros(8, dtype=np.uint64)
    return (O.msm_naive(scalars, bases) if len(bases) < 4096 else O.msm(scalars, bases, threads=8)).reshape(8)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 255, 4097, 70_000])
def test_msm_points_is_the_oracles(api, O, n):
    from halo2_vectordb_amd import verifier
    rng = np.random.default_rng(1000 + n)
    bases = _points_array(O, _random_points(rng, n))
    scalars = O.random_fr(rng, n).reshape(-1, 4)
    if n >= 3:                     # identity points, zero scalars, scalars r - 1
        bases[rng.choice(n, size=max(1, n // 50), replace=False)] = 0
        scalars[rng.choice(n, size=max(1, n // 50), replace=False)] = 0
        scalars[rng.choice(n, size=max(1, n // 50), replace=False)] = O.fr_from_ints([O.R_MOD - 1])[0]
    got = verifier.msm_points(bases, scalars)
    assert np.array_equal(got, _msm_want(O, scalars, bases))


@pytest.mark.parametrize("n", [255, 4097])
def test_msm_points_in_the_exceptional_cases(api, O, n):
    """every point equal (each bucket doubles), P beside -P (each bucket cancels to the identity), every scalar r - 1"""
    from halo2_vectordb_amd import verifier
    rng = np.random.default_rng(n)
    (x, y), = _random_points(rng, 1)
    P = _points_array(O, [(x, y)])[0]
    nP = _points_array(O, [(x, Q_MOD - y)])[0]
    same = np.tile(P, (n, 1))
    scalars = O.random_fr(rng, n).reshape(-1, 4)
    assert np.array_equal(verifier.msm_points(same, scalars), _msm_want(O, scalars, same))
    alt = np.stack([P if i % 2 == 0 else nP for i in range(n)])
    one = np.tile(O.fr_from_ints([7])[0], (n, 1))
    assert np.array_equal(verifier.msm_points(alt, one), _msm_want(O, one, alt))
    top = np.tile(O.fr_from_ints([O.R_MOD - 1])[0], (n, 1))
    assert np.array_equal(verifier.msm_points(alt, top), _msm_want(O, top, alt))
    pts = _points_array(O, _random_points(rng, n))
    assert np.array_equal(verifier.msm_points(pts, top), _msm_want(O, top, pts))
    assert np.array_equal(verifier.msm_points(pts, scalars), _msm_want(O, scalars, pts))


# ---- vdb_msm_points_dev at every window width ----------------------------------------------------------------------------------------
# The expected sum never forms a bucket: the points come from a pool of 8 curve points (and the identity) with random signs, so
#   sum_i s_i P_i = sum_j (sum_{i: P_i = +-pool_j} +-s_i mod r) pool_j
# is eight scalar multiplications over Python integers (the chord-and-tangent law of tests/l9_model.py).
R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
WIDTHS = list(range(4, 14))
SEG = 32                     # k_vmsm_segment's run of buckets


def _width_n(c):
    """the point count that makes vdb_msm_points_dev pick the window width c (vmsm_window: 4 below 256, then floor(log2 n) - 3, at most 13)"""
    n = 255 if c == 4 else 1 << (c + 3)
    lg = n.bit_length() - 1
    assert min(lg - 3 if lg > 7 else 4, 13) == c
    return n


def _mont_rows(vals, mod, per_row):
    """integers -> Montgomery form, `per_row` field elements per row of uint64 limbs"""
    raw = b"".join((v * (1 << 256) % mod).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4 * per_row).copy()


def _point_row(pt):
    return np.zeros(8, dtype=np.uint64) if pt is None else _mont_rows(pt, Q_MOD, 2)[0]


def _structured_scalars(c):
    """(tag, canonical scalar) for width c: W = ceil(254 / c) windows, the top one holding 254 - (W - 1) c bits"""
    W = -(-254 // c)
    top = 254 - (W - 1) * c
    assert 0 < top < c and W * c > 254
    out = [("all-ones", ((1 << 254) - 1) % R_MOD), ("all-ones", R_MOD - 1)]
    for name, w in (("first", 0), ("last-full", W - 2), ("top", W - 1)):
        width = top if w == W - 1 else c
        for d in (1, (1 << c) - 1, SEG - 1, SEG, SEG + 1):
            if d < 1 << width and d << (w * c) < R_MOD:
                out.append((f"digit-{name}", d << (w * c)))
    fill = ((1 << top) - 1) << ((W - 1) * c)               # every bit of the top window; reduced when it is not below r
    out.append(("top-fill", fill % R_MOD))
    out.append(("top-max", (R_MOD - 1) >> ((W - 1) * c) << ((W - 1) * c)))        # the largest top digit a canonical scalar has
    for w in range(W - 1):
        if (w * c) % 32 + c > 32:                            # the digit's bits lie in two 32-bit limbs
            out += [("straddle", d << (w * c)) for d in ((1 << c) - 1, 1 | 1 << (c - 1))]
    assert all(0 < s < R_MOD for _, s in out)
    have = {t for t, _ in out}
    assert {"all-ones", "digit-first", "digit-last-full", "digit-top", "top-fill", "top-max"} <= have, (c, have)
    assert ("straddle" in have) == (32 % c != 0)            # c-bit windows tile the 32-bit limbs exactly when c divides 32
    return out


@pytest.fixture(scope="module")
def msm_pool():
    import random

    import l9_model as L
    rng = random.Random(254)
    pool = [(1, 2)] + [L.ec_point(rng) for _ in range(7)]
    assert len({p[0] for p in pool}) == 8
    rows = np.stack([_point_row(p) for p in pool] + [_point_row(L.ec_neg(p)) for p in pool] + [_point_row(None)])
    return L, pool, rows


@pytest.mark.parametrize("c", WIDTHS)
def test_msm_points_at_every_window_width(api, msm_pool, c):
    """n = 255 (c = 4) and n = 2^(c + 3): structured scalars — every digit all-ones; one non-zero digit 1, 2^c - 1, 31, 32, 33 in the
    first, the last full and the top window; the top window filled; digits that straddle a 32-bit limb — then zero scalars on points,
    scalars on the identity, and random ones.  The pool is small, so every bucket that is hit holds repeated and opposite points"""
    from halo2_vectordb_amd import verifier
    L, pool, rows = msm_pool
    n = _width_n(c)
    rng = np.random.default_rng(7000 + c)
    structured = _structured_scalars(c)
    k = len(structured)
    assert k + 64 <= n
    which = rng.integers(0, 9, size=n)                     # 8: the identity
    which[:k] = np.arange(k) % 8                           # the structured scalars sit on points
    neg = rng.integers(0, 2, size=n)
    scalars = [s for _, s in structured] + [int.from_bytes(rng.bytes(32), "little") % R_MOD for _ in range(n - k)]
    zeros = [i for i in range(k, k + 32) if which[i] != 8][:8]
    for i in zeros:
        scalars[i] = 0
    assert zeros and any(which[i] == 8 and scalars[i] for i in range(n))
    coef = [0] * 8
    for j, s, sg in zip(which, scalars, neg):
        if j != 8:
            coef[j] = (coef[j] - s if sg else coef[j] + s) % R_MOD
    want = None
    for cj, p in zip(coef, pool):
        want = L.ec_add(want, L.ec_mul(cj, p))
    idx = np.where(which == 8, 16, which + 8 * neg)
    got = verifier.msm_points(rows[idx], _mont_rows(scalars, R_MOD, 1))
    print("cases:", n, "structured:", k)
    assert np.array_equal(got, _point_row(want))


@pytest.mark.parametrize("c", WIDTHS)
def test_msm_points_one_bucket_of_n_equal_points(api, msm_pool, c):
    """every point the same, every scalar 1: n P through one bucket of n equal additions (the first doubles)"""
    from halo2_vectordb_amd import verifier
    L, pool, rows = msm_pool
    n = _width_n(c)
    got = verifier.msm_points(np.tile(rows[c % 8], (n, 1)), np.tile(_mont_rows([1], R_MOD, 1)[0], (n, 1)))
    print("cases:", n)
    assert np.array_equal(got, _point_row(L.ec_mul(n, pool[c % 8])))


def _yardstick_vk(pr, out):
    from oracle import pairing as PR
    return dict(meta=_meta(pr), opened=out["opened"], fixed={name: pr.fixed[name].commits for name in FIXED}, tau_h=PR.pt_mul(PR.G2, TAU),
                instances=out["instances"])


def _tampered_cases(proof, meta):
    """test_a_verifier_accepts_the_proof_bytes_and_rejects_tampered_ones's byte flips, truncation and extension"""
    n_h = meta["chunk_len"] + 1
    n_points = meta["n_cols"] + 3 * meta["n_lk"] + meta["n_sets"] + 1 + n_h
    for where in (5, 32 * (n_points - n_h - 1) + 3, 32 * (n_points - 1) + 3, 32 * n_points + 40, len(proof) - 96 + 9, len(proof) - 64 + 7, len(proof) - 20):
        bad = bytearray(proof)
        bad[where] ^= 4
        yield bytes(bad)
    yield proof[:-32]
    yield proof + bytes(32)


def _wrong_keys(vk):
    from halo2_vectordb_amd.verifier import VerifyingKey
    meta = vk.meta
    for wrong in (w for w in (1, 2, 3) if w != meta["chunk_len"]):     # another constraint degree than the circuit's
        n_sets = -(-(meta["n_cols"] + 2) // wrong)
        yield VerifyingKey({**meta, "chunk_len": wrong}, vk.fixed, vk.opened, tau_g2=vk.tau_g2)
        yield VerifyingKey({**meta, "chunk_len": wrong, "n_sets": n_sets}, vk.fixed, vk.opened, tau_g2=vk.tau_g2)
    yield VerifyingKey({**meta, "n_blind": meta["n_blind"] - 1}, vk.fixed, vk.opened, tau_g2=vk.tau_g2)


def _accepts_and_rejects_like_the_yardstick(api, O, pr, out):
    from halo2_vectordb_amd import verifier
    vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
    proof, inst = out["proof"], out["instances"]
    yvk = _yardstick_vk(pr, out)
    assert _verify(O, api, proof, yvk) and verifier.verify(proof, inst, vk)
    assert not verifier.verify(proof, [], vk)
    other = list(inst)
    other[0] = (other[0] + 1) % O.R_MOD
    assert not verifier.verify(proof, other, vk)
    for bad in _tampered_cases(proof, vk.meta):
        assert not verifier.verify(bad, inst, vk)
    for wrong in _wrong_keys(vk):
        assert not verifier.verify(proof, inst, wrong)
    return vk


@pytest.fixture(scope="module")
def kmeans(api):
    from halo2_vectordb_amd.pipeline import KmeansHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    hp = KmeansHotPath(n=8, dim=4, K=2, I=1, k=12, L=11, metric="cosine", tau=TAU).setup()
    pr = ProverRounds(hp).keygen()
    assert pr.keygen_report.violations() == 0
    yield hp, pr, pr.prove(None, seed=31)
    pr.free()
    hp.free()


def test_kmeans_proof_accepted_and_tampering_rejected(api, O, kmeans):
    _hp, pr, out = kmeans
    _accepts_and_rejects_like_the_yardstick(api, O, pr, out)


def test_random_byte_flips_get_the_yardsticks_verdict(api, O, kmeans):
    """64 seeded single-byte changes: the same verdict as _verify.  One deliberate difference: the yardstick's decoder ignores bit 7
    of a point's last byte under the bit-6 convention, the product rejects it (x would not be canonical) — a change of that bit
    alone is the only place the two may differ, and there only the product may reject."""
    from halo2_vectordb_amd import verifier
    _hp, pr, out = kmeans
    vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
    proof, inst, yvk = out["proof"], out["instances"], _yardstick_vk(pr, out)
    rng = np.random.default_rng(64)
    for _ in range(64):
        where, mask = int(rng.integers(len(proof))), int(rng.integers(1, 256))
        bad = bytearray(proof)
        bad[where] ^= mask
        mine, theirs = verifier.verify(bytes(bad), inst, vk), _verify(O, api, bytes(bad), yvk)
        if mask == 0x80 and where % 32 == 31:
            assert not mine
        else:
            assert mine == theirs, (where, mask)


def test_merkle_proof_accepted_and_tampering_rejected(api, O):
    from halo2_vectordb_amd.pipeline import MerkleHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    hp = MerkleHotPath(n=6, dim=5, k=11, tau=TAU).setup()
    pr = ProverRounds(hp).keygen()
    try:
        assert pr.n_lk == 0
        _accepts_and_rejects_like_the_yardstick(api, O, pr, pr.prove(None, seed=4))
    finally:
        pr.free()
        hp.free()


def test_query_proof_accepted_and_tampering_rejected(api, O):
    from halo2_vectordb_amd.pipeline import QueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    hp = QueryHotPath(n=6, dim=4, k=12, L=11, metric="cosine", tau=TAU).setup()
    pr = ProverRounds(hp).keygen()
    try:
        assert pr.keygen_report.violations() == 0
        _accepts_and_rejects_like_the_yardstick(api, O, pr, pr.prove(None, seed=17))
    finally:
        pr.free()
        hp.free()


def _cli(*args):
    from halo2_vectordb_amd import verify as cli
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = cli.main([str(a) for a in args])
    return rc, json.loads(buf.getvalue())


def test_from_files_and_the_command_line(api, O, kmeans, tmp_path):
    from halo2_vectordb_amd.io import read_snark, write_snark
    from halo2_vectordb_amd.verifier import Verifier
    _hp, pr, out = kmeans
    snark = str(tmp_path / "kmeans.snark")
    write_snark(snark, out["proof"], out["instances"])
    pr.save_verifying_key(snark + ".vk.npz", opened=out["opened"])
    pr.save_verifying_key_raw(str(tmp_path / "kmeans.vk"))
    v = Verifier.from_files(snark, snark + ".vk.npz")
    assert v.proof == out["proof"] and v.instances == out["instances"] and v.verify()
    assert Verifier.from_files(snark, str(tmp_path / "kmeans.vk"), tau=TAU).verify()
    assert not Verifier.from_files(snark, str(tmp_path / "kmeans.vk"), tau=TAU + 1).verify()
    rc, rep = _cli(snark, snark + ".vk.npz")
    assert rc == 0 and rep["accepted"] is True and rep["verify_s"] > 0
    assert _cli(snark, tmp_path / "kmeans.vk", hex(TAU))[0] == 0
    proof, inst = read_snark(snark)
    bad = bytearray(proof)
    bad[len(bad) // 3] ^= 2
    write_snark(str(tmp_path / "bad.snark"), bytes(bad), inst)
    rc, rep = _cli(tmp_path / "bad.snark", snark + ".vk.npz")
    assert rc == 1 and rep["accepted"] is False
    # a key whose stored digest is not its commitments' digest is not a key
    with np.load(snark + ".vk.npz") as doc:
        d = dict(doc)
    meta = json.loads(bytes(d["meta"]).decode())
    meta["vk_digest"] = str(int(meta["vk_digest"]) + 1)
    d["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez(str(tmp_path / "forged.vk.npz"), **d)
    with pytest.raises(ValueError):
        Verifier.from_files(snark, str(tmp_path / "forged.vk.npz"))
    assert _cli(snark, tmp_path / "forged.vk.npz")[0] == 1


def test_c4_cosine_full_size_verifies(api, O, tmp_path):
    """C4' (tests/test_gpu_c4_full.py, tools/c4_cosine.py): 20,969 columns, ~58 k commitments between the proof and the key"""
    import time
    from halo2_vectordb_amd.io import write_snark
    from halo2_vectordb_amd.pipeline import KmeansHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    from halo2_vectordb_amd.verifier import Verifier
    hp = KmeansHotPath(seed=20260004, metric="cosine", n=256, dim=128, K=4, I=8, k=16, P=48, L=15)
    hp.ext_block_cols = 256
    hp.setup()
    pr = None
    try:
        assert hp.n_cols == 20_969
        pr = ProverRounds(hp).keygen()
        out = pr.prove(None)
        path = str(tmp_path / "c4.snark")
        write_snark(path, out["proof"], out["instances"])
        pr.save_verifying_key(path + ".vk.npz", opened=out["opened"])
        proof = out["proof"]
        del out
    finally:
        if pr is not None:
            pr.free()
        hp.free()
        from halo2_vectordb_amd._lib import check
        check(api.init().vdb_scratch_release())
    v = Verifier.from_files(path, path + ".vk.npz")
    t0 = time.perf_counter()
    ok = v.verify()
    wall = time.perf_counter() - t0
    print(json.dumps({"c4_verify_s": round(wall, 4), "stages_s": {k: round(s, 4) for k, s in v.timings.items()}, "proof_bytes": len(proof)}))
    assert ok
    bad = bytearray(proof)
    bad[len(bad) // 3] ^= 2
    v.proof = bytes(bad)
    assert not v.verify()
