"""Python model of the MSM driver's planner (halo2_vectordb_amd/csrc/msm_plan.hpp), shared by tests/test_msm_plan_cpu.py — which holds
`tools/msm_plan_probe.hip --host` to it word for word — and tests/test_gpu_msm_plan.py, which counts the driver's launches against it.

Written from the driver as it stood before the planner was split out of it: one function body that picked the range length, summed the
bytes of a column by hand (`n * 12`: eight bytes of record and four of queue per scalar), clamped a budget, turned it into a batch size
and carved the work space by pointer arithmetic, `+ 512` for the 64 counter words, the alignment of the records and slack.  The one
thing stated here that the old carve did not do: every region starts on a multiple of its element's alignment (ALIGN), the padding coming
out of the 512 bytes."""
import collections
import functools

MAGIC = 0x4D53504C
NIN = [12, 15]          # words of a case of op 0 (by window) and op 1 (by shape)
NMSG = 24
REGIONS = ["entries", "raw", "sums", "ranges", "seginfo", "seg_off", "bucket_off", "counters", "recs", "longq"]
ALIGN = dict(entries=4, raw=16, sums=16, ranges=4, seginfo=4, seg_off=4, bucket_off=4, counters=4, recs=8, longq=4)
NOUT = 2 + NMSG + 5 + 1 + 6 + 2 + 4 + 3 + 6 + 2 * len(REGIONS)
OK, REFUSED = 0, -3     # VDB_OK, VDB_ERR_ARG (include/vdb.h)
GIB = 1 << 30
LDS_MAX = 160 * 1024

RANGE_BYTES, SEGINFO_BYTES, RAW_BYTES = 24, 8, 36 * 4      # MsmRange, MsmSegInfo, one raw record
SORT_THREADS, SCATTER2_THREADS, BIN_CAP = 1024, 256, 6 * 1024
COUNTER_WORDS, SLACK = 64, 512

Shape = collections.namedtuple("Shape", "c W B table_n")
Mem = collections.namedtuple("Mem", "free held cap", defaults=(0, 0))


def window(k, window_bits=0, knob=0):
    """-> (rc, why, Shape): vdb_srs_load_window's choice of c, W and B.  `knob`: VDB_MSM_C as an integer, 0 when unset"""
    if not (window_bits == 0 or 2 <= window_bits <= 14):
        return REFUSED, "window_bits must be 0 (default) or 2..14", None
    c = window_bits or (knob if 2 <= knob <= 14 else (8 if k <= 8 else 11))
    W = (254 + c - 1) // c
    if W << k > 0x7FFFFFFF:
        return REFUSED, "srs: table index does not fit 31 bits", None
    return OK, "", Shape(c, W, 1 << (c - 1), 1 << k)


def budget(mem):
    """half of what is free counting what the slot holds, 8 .. 96 GiB; under a cap, the cap or what is held already"""
    b = min(max((mem.free + mem.held) // 2, 8 * GIB), 96 * GIB)
    if mem.cap and b > mem.cap:
        b = max(mem.cap, mem.held)
    return b


class Plan:
    def __init__(self, rc, why="", **fields):
        self.rc, self.why = rc, why
        self.__dict__.update(fields)

    def region_bytes(self, name):
        """what the kernels may touch of a region"""
        per_col = dict(entries=4 * self.ent_cap, raw=RAW_BYTES * self.seg_cap_col, sums=RAW_BYTES, ranges=RANGE_BYTES * self.range_cap_col,
                       seginfo=SEGINFO_BYTES * self.seg_cap_col, seg_off=4 * (self.shape.B + 1), bucket_off=4 * (self.shape.B + 1), counters=0,
                       recs=8 * self.n, longq=4 * self.n)[name]
        return self.nb * per_col + (4 * COUNTER_WORDS if name == "counters" else 0)


@functools.lru_cache(maxsize=None)
def _plan(shape, n_cols, n, budget_bytes):
    c, W, B, table_n = shape
    if n_cols == 0 or n == 0 or n > table_n:
        return Plan(REFUSED, "msm: the job does not fit the loaded table")
    ent_cap = n * W
    lcap = 32
    while lcap < 256 and (n_cols * n) // lcap >= 1 << 19:
        lcap <<= 1
    range_cap_col = -(-ent_cap // lcap)
    seg_cap_col = B + range_cap_col
    per_col = ent_cap * 4 + range_cap_col * RANGE_BYTES + seg_cap_col * (SEGINFO_BYTES + RAW_BYTES) + RAW_BYTES + 2 * (B + 1) * 4 + n * 12
    idx_bits = 1
    while idx_bits < 32 and 1 << idx_bits < W * table_n:
        idx_bits += 1
    fine_bits = 0
    if c >= 13:
        fine_bits = c - 1 - 8
        if fine_bits + idx_bits > 31:
            fine_bits = 31 - idx_bits if idx_bits < 31 else 0
        if fine_bits < 2:
            fine_bits = 0
    if fine_bits + idx_bits > 31:
        return Plan(REFUSED, "msm: table index and fine bucket number do not fit an entry's 31 bits")
    sort_lds = (3 * B + 32) * 4
    scatter2_lds = (BIN_CAP + (1 << fine_bits)) * 4 if fine_bits else 0
    if max(sort_lds, scatter2_lds) > LDS_MAX:
        return Plan(REFUSED, "msm: a kernel needs more than 160 KiB of LDS")
    nb = min(max(budget_bytes // per_col, 1), n_cols, 16384)
    if nb * seg_cap_col > 0x7FFFFFFF:
        nb = 0x7FFFFFFF // seg_cap_col
    passes = 0
    while 1 << passes < range_cap_col + 1:
        passes += 1
    P = Plan(OK, shape=shape, n_cols=n_cols, n=n, lcap=lcap, ent_cap=ent_cap, range_cap_col=range_cap_col, seg_cap_col=seg_cap_col,
             seg_cap=nb * seg_cap_col, range_cap=nb * range_cap_col, idx_bits=idx_bits, fine_bits=fine_bits, bin_cap=BIN_CAP,
             scatter2_bins_x=min(B >> fine_bits, 64) if fine_bits else 0, sort_lds=sort_lds, scatter2_lds=scatter2_lds,
             combine_passes=passes, nb=nb, n_batches=-(-n_cols // nb), bytes=nb * per_col + SLACK, per_col=per_col)
    # the carve, in the old order: entries, raw, sums, ranges, seginfo, seg_off, bucket_off, 64 counter words, records, queue
    P.off, at = {}, 0
    for name in REGIONS:
        at = -(-at // ALIGN[name]) * ALIGN[name]
        P.off[name] = at
        at += P.region_bytes(name)
    P.end = at
    return P


def plan(shape, n_cols, n, mem=Mem(200 * GIB)):
    return _plan(shape, n_cols, n, budget(mem))


# ---- the probe's words ---------------------------------------------------------------------------------------------------------------
def w64(v):
    return [v & 0xFFFFFFFF, v >> 32]


def case_words(k, window_bits, n, n_cols, mem):
    return [k, window_bits] + w64(n) + w64(n_cols) + w64(mem.free) + w64(mem.held) + w64(mem.cap)


def shape_case_words(shape, n, n_cols, mem):
    return [shape.c, shape.W, shape.B] + w64(shape.table_n) + w64(n) + w64(n_cols) + w64(mem.free) + w64(mem.held) + w64(mem.cap)


def msg_words(why):
    msg = why.encode()
    assert len(msg) <= 4 * NMSG
    msg += bytes(4 * NMSG - len(msg))
    return [int.from_bytes(msg[4 * i: 4 * i + 4], "little") for i in range(NMSG)]


@functools.lru_cache(maxsize=None)
def _expect(rc_w, why_w, shape, P):
    if rc_w != OK:
        out = [rc_w & 0xFFFFFFFF, 0] + msg_words(why_w)
        return out + [0] * (NOUT - len(out))
    out = [0, P.rc & 0xFFFFFFFF] + msg_words(P.why) + [shape.c, shape.W, shape.B] + w64(shape.table_n)
    if P.rc == OK:
        out += ([P.lcap] + w64(P.ent_cap) + w64(P.range_cap_col) + w64(P.seg_cap_col) +
                [P.seg_cap, P.range_cap, P.idx_bits, P.fine_bits, P.bin_cap, P.scatter2_bins_x, P.sort_lds, P.scatter2_lds, P.combine_passes] +
                w64(P.nb) + w64(P.n_batches) + w64(P.bytes))
        for name in REGIONS:
            out += w64(P.off[name])
    return out + [0] * (NOUT - len(out))


def expect_words(rc_w, why_w, shape, P):
    """the probe's record for a case: msm_window's answer (rc_w, why_w, shape) and, where it gave a shape, the plan"""
    return _expect(rc_w, why_w, shape, P)
