"""Python model of the NTT driver's planner (halo2_vectordb_amd/csrc/ntt_plan.hpp), shared by tests/test_ntt_plan_cpu.py — which holds
`tools/ntt_plan_probe.hip --host` to it word for word — and tests/test_gpu_ntt_plan.py, which counts the driver's launches against it.

Written from what the header promises, with exact numbers where the header has doubles: the limb-bound walk runs in
fractions.Fraction, cmax is the largest of limbs 0..7 of l9_model.offset_limbs(14, R) over 2^29, and the thresholds are 1.0001 =
10001/10000, 6.1 = 61/10 and 7.95 = 159/20.  `walk` records every comparison's distance from its threshold, every bound that enters a
product and every bound a limb reaches, so the test can state that doubles and fractions cannot disagree and that the schedule is safe."""
import collections
import functools
from fractions import Fraction

import l9_model as L

MAGIC = 0x4E54504C
MAX_PASSES = 4
NIN, NMSG, NPASS = 7, 24, 28
NOUT = 1 + NMSG + 4 + 9 + MAX_PASSES * NPASS
OK, REFUSED = 0, -3     # VDB_OK, VDB_ERR_ARG (include/vdb.h)

Knobs = collections.namedtuple("Knobs", "max_s shoup spec shoup_all blk0", defaults=(9, True, True, True, True))
Job = collections.namedtuple("Job", "log_n in_len n_cols vslots scale_ninv coset_in has_in_scale coset_out has_in_tabs has_srcs in_place",
                             defaults=(0, 2, 0, False, False, False, False, False, False, False))

# the k_ntt_pass instantiations in the order of the header's enum: name, (LAST, VS, CS, CS0, CREN, SA)
KERNELS = [("LAST_VS", (1, 1, 0, 0, 0, 0)), ("LAST_256_SA", (1, 0, 8, 0, 4, 1)), ("LAST_512_SA", (1, 0, 9, 0, 20, 1)),
           ("LAST_256", (1, 0, 8, 0, 4, 0)), ("LAST_512", (1, 0, 9, 0, 20, 0)), ("LAST", (1, 0, 0, 0, 0, 0)),
           ("VS_256", (0, 1, 8, 0, 4, 0)), ("VS", (0, 1, 0, 0, 0, 0)), ("256_SA", (0, 0, 8, 0, 4, 1)), ("512_PAD_SA", (0, 0, 9, 2, 4, 1)),
           ("512_SA", (0, 0, 9, 0, 20, 1)), ("256", (0, 0, 8, 0, 4, 0)), ("512_PAD", (0, 0, 9, 2, 4, 0)), ("512", (0, 0, 9, 0, 20, 0)),
           ("GENERIC", (0, 0, 0, 0, 0, 0))]
KERNEL_ID = {name: i for i, (name, _) in enumerate(KERNELS)}

CKP = L.offset_limbs(14, L.R)
CMAX = Fraction(max(CKP[:8]), L.B29)
RENORMED, PRODUCT_MAX, LIMB_MAX = Fraction(10001, 10000), Fraction(61, 10), Fraction(159, 20)

Walk = collections.namedtuple("Walk", "ren_mask final products bounds margins")


def spec_sh_res_log(cs, sa):
    """the Shoup table resolution a specialised k_ntt_pass instantiation takes for itself (ntt_spec_sh_res_log)"""
    return 0 if cs == 8 else (1 if sa else 2)


@functools.lru_cache(maxsize=None)
def walk(S, s0):
    """the carry-pass schedule of a pass of 2^S points from stage s0.  Limb bounds in units of 2^29: a value comes out of a carry pass
    below RENORMED and is loaded below 1; a sum adds the operands' bounds, a difference adds CMAX.  A radix-4 step multiplies its
    operands (bound b) and then the results of its first stage (b + CMAX); a radix-2 step multiplies its operands."""
    b, mask, step, st = RENORMED, 0, 0, s0
    products, bounds, margins = [], [], []

    def at_least(x, t):
        margins.append(abs(x - t))
        return x >= t

    while st < S:
        two = st + 1 < S
        grow = (2 if two else 1) * CMAX
        if st == 0:
            b = Fraction(1)
        elif (at_least(b + CMAX, PRODUCT_MAX) if two else at_least(b, PRODUCT_MAX)) or at_least(b + grow, LIMB_MAX):
            mask |= 1 << step
            b = RENORMED
        if st > 0:
            products.append(b)
        if two:
            products.append(b + CMAX)
        b += grow
        bounds.append(b)
        st += 2 if two else 1
        step += 1
    return Walk(mask, b, tuple(products), tuple(bounds), tuple(margins))


def pass_sizes(log_n, max_s):
    if log_n <= 10:
        return [log_n]
    ms = max_s if 4 <= max_s <= 9 else 9
    while -(-log_n // ms) > MAX_PASSES:
        ms += 1
    n_passes = -(-log_n // ms)
    return [log_n // n_passes + (1 if l < log_n % n_passes else 0) for l in range(n_passes)]


class Plan:
    """rc and why, and for rc == OK: L, passes (one dict per pass, the fields of NttPassPlan plus its `walk`), needs_scaled_twiddles"""

    def __init__(self, job, rc, why="", passes=()):
        self.job, self.rc, self.why, self.passes, self.L = job, rc, why, list(passes), len(passes)
        self.needs_scaled_twiddles = bool(job.scale_ninv and self.L > 1)

    def chunk_cols(self, n_cols):
        if self.L == 1:
            return n_cols
        chunk = min(n_cols, max(1, (2 << 30) // (32 << self.job.log_n)))
        v = self.job.vslots
        return (chunk // v * v or v) if v else chunk

    def chunks(self, n_cols):
        return -(-n_cols // self.chunk_cols(n_cols))


def plan(job, kn=Knobs()):
    j = job
    refuse = lambda why: Plan(j, REFUSED, why)
    if j.log_n > 26:
        return refuse("ntt: log_n > 26 unsupported")
    n = 1 << j.log_n
    in_len = j.in_len or n
    if j.in_place and in_len != n:
        return refuse("ntt: in-place transform needs in_len == n")
    if j.vslots and (j.in_place or not j.has_in_tabs or j.vslots > 4 or j.has_srcs or j.coset_in or j.n_cols % j.vslots):
        return refuse("ntt: virtual columns need an output buffer and their input tables")
    if j.has_srcs and (j.in_place or in_len != n or j.log_n <= 10):
        return refuse("ntt: column sources need an output buffer and a multi-pass size")
    S = pass_sizes(j.log_n, kn.max_s)
    n_passes, passes, done = len(S), [], 0
    for l, s in enumerate(S):
        first, last = l == 0, l == n_passes - 1
        vs = first and j.vslots > 0
        p = dict(S=s, log_inner=j.log_n - done - s, first=first, last=last)
        done += s
        p["coset"] = (2 if j.has_in_scale else 1) if first and j.coset_in else (3 if vs else 0)
        p["scale"] = int(last and j.scale_ninv and n_passes == 1)
        p["coset_out"] = int(last and j.coset_out)
        p["s0"] = 2 if first and not last and S[0] >= 3 and in_len * 4 <= n else 0
        w = walk(s, p["s0"])
        p["walk"], p["ren_mask"] = w, w.ren_mask
        if p["s0"] == 0 and w.ren_mask & 1:
            return refuse("ntt: the carry schedule put a carry pass in front of the step at stage 0")
        p["out_mul"] = not last or bool(p["scale"]) or bool(p["coset_out"])
        p["blk0"] = int(kn.blk0)
        p["ren_out"] = int(p["out_mul"] and w.final >= PRODUCT_MAX)
        m = 1 << s
        p["logG"] = min(10 - s, S[0] if last else p["log_inner"]) if n_passes > 1 else 0
        p["nprev"] = l if n_passes > 1 else 0
        p["prevS"] = (S[:l] if n_passes > 1 else []) + [0] * (MAX_PASSES - (l if n_passes > 1 else 0))
        G = 1 << p["logG"]
        p["tiles"] = n // (m * G)

        def spec_shape(cs, cs0, cren):
            return kn.spec and n_passes > 1 and (s, p["s0"], w.ren_mask, p["logG"]) == (cs, cs0, cren, 10 - cs) and kn.blk0

        sa = bool(kn.shoup_all and kn.shoup and not vs and j.log_n <= 22 and
                  (spec_shape(8, 0, 4) or spec_shape(9, 0, 20) or (not last and spec_shape(9, 2, 4))))
        lds = (G * (m + 1) + (0 if sa else max(m // 2, 1))) * 36      # two 16-byte planes and a 4-byte one
        p.update(sa=sa, has_sh_tab=False, sh_res_log=0, sh_ns=0, sh_max_s=-1)
        if kn.shoup and s >= 4:
            room, rl = 160 * 1024 // 3, 0
            while rl + 2 < s and lds + ((m // 2) >> rl) * 72 > room:
                rl += 1
            if lds + ((m // 2) >> rl) * 72 <= room and s - 2 - rl >= 1:
                p.update(has_sh_tab=True, sh_res_log=rl, sh_ns=(m // 2) >> rl, sh_max_s=s - 2 - rl)
                lds += p["sh_ns"] * 72
        if lds > 64 * 1024:
            return refuse("ntt: a pass needs more than 64 KiB of LDS")
        p["lds_bytes"] = lds

        def spec(cs, cs0, cren, sa_):
            rl = spec_sh_res_log(cs, sa_)
            return (spec_shape(cs, cs0, cren) and p["has_sh_tab"] and
                    (p["sh_res_log"], p["sh_ns"], p["sh_max_s"]) == (rl, (1 << (cs - 1)) >> rl, cs - 2 - rl))

        if sa and not spec(s, p["s0"], w.ren_mask, True):
            return refuse("ntt: SA plan does not match its instantiation")
        p["needs_sh2_tab"], p["needs_tw_rec"] = bool(sa and s & 1), bool(sa and not last)
        if last:
            k = ("LAST_VS" if vs else "LAST_256_SA" if sa and s == 8 else "LAST_512_SA" if sa else
                 "LAST_256" if spec(8, 0, 4, False) else "LAST_512" if spec(9, 0, 20, False) else "LAST")
        else:
            k = ("VS_256" if vs and spec(8, 0, 4, False) else "VS" if vs else "256_SA" if sa and s == 8 else
                 "512_PAD_SA" if sa and p["s0"] == 2 else "512_SA" if sa else "256" if spec(8, 0, 4, False) else
                 "512_PAD" if spec(9, 2, 4, False) else "512" if spec(9, 0, 20, False) else "GENERIC")
        p["kernel"] = k
        passes.append(p)
    return Plan(j, OK, passes=passes)


# ---- the probe's words ---------------------------------------------------------------------------------------------------------------
def knob_word(kn):
    return kn.max_s | int(kn.shoup) << 8 | int(kn.spec) << 9 | int(kn.shoup_all) << 10 | int(kn.blk0) << 11


def job_words(j):
    flags = (int(j.scale_ninv) | int(j.coset_in) << 1 | int(j.has_in_scale) << 2 | int(j.coset_out) << 3 | int(j.has_in_tabs) << 4 |
             int(j.has_srcs) << 5 | int(j.in_place) << 6)
    return [j.log_n, j.in_len & 0xFFFFFFFF, j.in_len >> 32, j.n_cols & 0xFFFFFFFF, j.n_cols >> 32, j.vslots, flags]


def expect_words(P):
    out = [P.rc & 0xFFFFFFFF]
    msg = P.why.encode()
    assert len(msg) <= 4 * NMSG
    msg += bytes(4 * NMSG - len(msg))
    out += [int.from_bytes(msg[4 * i: 4 * i + 4], "little") for i in range(NMSG)]
    if P.rc != OK:
        return out + [0] * (NOUT - len(out))
    chunk = P.chunk_cols(P.job.n_cols)
    out += [P.L, int(P.needs_scaled_twiddles), chunk & 0xFFFFFFFF, chunk >> 32] + CKP
    for p in P.passes:
        out += [p["S"], p["log_inner"], int(p["first"]), int(p["last"]), p["coset"], p["s0"], p["ren_mask"], p["ren_out"], p["blk0"], p["scale"],
                p["coset_out"], p["logG"], p["nprev"]] + p["prevS"] + [p["tiles"], p["lds_bytes"], int(p["has_sh_tab"]), p["sh_res_log"],
                                                                        p["sh_ns"], p["sh_max_s"] & 0xFFFFFFFF, int(p["sa"]), int(p["needs_sh2_tab"]),
                                                                        int(p["needs_tw_rec"]), KERNEL_ID[p["kernel"]], spec_sh_res_log(p["S"], p["sa"])]
    return out + [0] * (NOUT - len(out))


# ---- the jobs of the driver's callers ------------------------------------------------------------------------------------------------
def caller_jobs(log_n, n_cols=12):
    """what the entry points of ntt.hip ask for at this size (and what they would ask for at input lengths they do not use today)"""
    n = 1 << log_n
    J = lambda **kw: Job(log_n=log_n, n_cols=n_cols, **kw)
    jobs = [("ntt_batch", J(in_place=True)),
            ("ntt_batch inverse / lagrange_to_coeff / cosets_to_coeff", J(in_place=True, scale_ninv=True)),
            ("extended_to_coeff", J(in_place=True, scale_ninv=True, coset_out=True)),
            ("ntt_batch, in_len == n given", J(in_place=True, in_len=n))]
    for in_len in sorted({n, max(n // 2, 1), max(n // 4, 1), max(n // 8, 1), 1}, reverse=True):
        jobs += [(f"out of place, in_len {in_len}", J(in_len=in_len)),
                 (f"out of place inverse, in_len {in_len}", J(in_len=in_len, scale_ninv=True)),
                 (f"coeff_to_extended, in_len {in_len}", J(in_len=in_len, coset_in=True)),
                 (f"coeff_to_extended_scaled, in_len {in_len}", J(in_len=in_len, coset_in=True, has_in_scale=True)),
                 (f"lagrange_to_coeff_src, in_len {in_len}", J(in_len=in_len, scale_ninv=True, has_srcs=True))]
        jobs += [(f"coeff_to_cosets, {v} slots, in_len {in_len}", J(in_len=in_len, vslots=v, has_in_tabs=True)) for v in (1, 3, 4)]
    return jobs
