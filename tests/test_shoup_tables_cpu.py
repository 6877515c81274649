"""The Shoup companions of the NTT's constant multiplicands (halo2_vectordb_amd/csrc/shoup_tables.hpp: the stage tables, the inter-pass
records the device builds from the twiddle tables, the coset constants) held to Python's integers at k = 1 ... 20: every entry's w is
the canonical residue it stands for and w' = floor(w 2^261 / r).  The host build of the same functions (tools/shoup_tables.hip)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def companion(w):
    return (w << 261) // R


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_shoup_companions_against_python_integers(tmp_path):
    from oracle import oracle as O
    ZETA = O.fr_to_ints(O.zeta().reshape(1, 4))[0]
    assert pow(ZETA, 3, R) == 1 and ZETA != 1
    exe = str(tmp_path / "shoup_tables")
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-o", exe,
                           os.path.join(ROOT, "tools", "shoup_tables.hip")], stderr=subprocess.DEVNULL)
    ks = range(1, 21)
    omegas = {k: O.fr_to_ints(O.root_of_unity(k).reshape(1, 4))[0] for k in ks}
    assert all(pow(w, 1 << k, R) == 1 and pow(w, 1 << (k - 1), R) != 1 for k, w in omegas.items())
    # the inverse transforms' tables are built from omega^-1: check those too
    inputs = [(k, w) for k in ks for w in (omegas[k], pow(omegas[k], -1, R))]
    stdin = "".join(f"{k} {w:x} {ZETA:x}\n" for k, w in inputs)
    out = subprocess.run([exe], input=stdin, capture_output=True, text=True, check=True).stdout.splitlines()
    # check block by block: split the output at the first line of each input's stage tables (S = 1, rl = 0, j = 0)
    blocks, cur = [], None
    for line in out:
        f = line.split()
        if f[0] == "st" and f[2:5] == ["1", "0", "0"]:
            cur = []
            blocks.append(cur)
        cur.append(f)
    assert len(blocks) == len(inputs)
    for (k, omega), lines in zip(inputs, blocks):
        n = 1 << k
        n_st = n_ip = n_c = 0
        for f in lines:
            assert int(f[1], 16) == k
            if f[0] == "st":
                S, rl, j = (int(x, 16) for x in f[2:5])
                w, q = int(f[5], 16), int(f[6], 16)
                e = j << rl
                assert w == pow(omega, (e * n) >> S, R), (k, S, rl, j)
                assert q == companion(w), (k, S, rl, j)
                n_st += 1
            elif f[0] == "ip":
                scaled, e = int(f[2], 16), int(f[3], 16)
                w, q = int(f[4], 16), int(f[5], 16)
                want = pow(omega, e, R) * (pow(n, -1, R) if scaled else 1) % R
                assert w == want, (k, scaled, e)
                assert q == companion(w), (k, scaled, e)
                assert f[6:8] == ["0", "0"]
                n_ip += 1
            else:
                i = int(f[2], 16)
                w, q = int(f[3], 16), int(f[4], 16)
                assert w == pow(ZETA, i, R) and q == companion(w), (k, i)
                n_c += 1
        S_max = min(k, 9)
        assert n_st == sum(((1 << S) // 2) >> rl for S in range(1, S_max + 1) for rl in range(min(3, S)))
        assert n_ip == 96 and n_c == 3
