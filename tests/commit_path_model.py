"""Plain reference of the commit path's column sources (include/vdb.h, vdb_colsrc) and of the MSM's signed-digit recoding: numpy and
Python integers only, no GPU, none of the project's kernels.  tests/test_commit_path_cpu.py checks it against itself and against the
oracle's column layout; tests/test_gpu_commit_path.py holds the library to it."""
import numpy as np

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
FR_BITS = 254


def windows(c):
    """number of c-bit windows of a scalar"""
    return (FR_BITS + c - 1) // c


# ------------------------------------------------------------------ columns that still lie in a stream
def materialise(stream, start, length, blind, n, n_blind):
    """The column a descriptor (stream + start, length, blind) stands for, n rows of 4 words: rows [0, length) are the stream cells
    from `start` on, the last n_blind rows are `blind` (n_blind x 4) when given, every other row is zero."""
    assert 0 <= length <= n and 0 <= n_blind <= n and start >= 0 and start + length <= len(stream)
    col = np.zeros((n, 4), dtype=np.uint64)
    col[:length] = stream[start:start + length]
    if blind is not None and n_blind:
        col[n - n_blind:] = np.asarray(blind, dtype=np.uint64).reshape(n_blind, 4)
    return col


def descriptors(n_cells, break_points, k, col_lo, col_hi):
    """(start, len) of the advice columns [col_lo, col_hi): column c starts where the break points before it add up to and holds
    break_points[c] + 1 cells (the cell on the break row is the first cell of the next column again); the column after the last
    break point holds the rest of the stream."""
    bp = [int(b) for b in break_points]
    rows = 1 << k
    assert 0 <= col_lo <= col_hi <= len(bp) + 1
    out = []
    for c in range(col_lo, col_hi):
        start = sum(bp[:c])
        length = bp[c] + 1 if c < len(bp) else n_cells - start
        assert bp[c] < rows if c < len(bp) else True
        assert 0 <= length <= rows and start + length <= n_cells
        out.append((start, length))
    return out


def descriptors_lookup(n_cells, k, minimum_rows, col_lo, col_hi):
    """(start, len) of the lookup columns [col_lo, col_hi): consecutive stretches of 2^k - minimum_rows cells; a column past the end
    of the stream is empty and points at the stream's base."""
    max_rows = (1 << k) - minimum_rows
    out = []
    for c in range(col_lo, col_hi):
        start = c * max_rows
        out.append((start, min(n_cells - start, max_rows)) if start < n_cells else (0, 0))
    return out


def const_mask(flags, n_cells, break_points, k):
    """column image ((n_bp + 1) x 2^k bytes) of bit 1 of the flag bytes, zero outside every column's cells"""
    rows = 1 << k
    desc = descriptors(n_cells, break_points, k, 0, len(break_points) + 1)
    out = np.zeros((len(desc), rows), dtype=np.uint8)
    for c, (start, length) in enumerate(desc):
        out[c, :length] = (np.asarray(flags[start:start + length], dtype=np.uint8) >> 1) & 1
    return out


# ------------------------------------------------------------------ signed-digit recoding
def signed_digits(s, c, W):
    """[(window j, signed digit d)] with d != 0 and s = sum d * 2^(c j) mod r: a scalar above (r - 1) / 2 is taken as -(r - s); the
    magnitude is cut into c-bit windows from the bottom; a window value (with the carry) above 2^(c-1) becomes its distance to 2^c,
    negative, and carries one into the next window."""
    s %= R
    sign = 1
    if s > (R - 1) // 2:
        s, sign = R - s, -1
    out, carry = [], 0
    for j in range(W):
        if not carry and not s >> (c * j):
            break                       # nothing but zero digits from here on
        d = ((s >> (c * j)) & ((1 << c) - 1)) + carry
        carry = 0
        if d > 1 << (c - 1):
            d -= 1 << c
            carry = 1
        if d:
            out.append((j, sign * d))
    assert carry == 0, "the top window cannot carry: the magnitude is below 2^253"
    return out


def count_entries(col, mask, c, W):
    """number of non-zero signed digits over the cells of `col` (canonical integers) that `mask` (bytes, or None) does not flag"""
    return sum(len(signed_digits(int(v), c, W)) for i, v in enumerate(col) if mask is None or not mask[i])


def edge_scalars(c):
    """what sits on the edges of the recoding with c-bit windows: the fold point, the short / long limit 2^32, and for every window j a
    digit that carries (2^(c j) - 1), the largest that does not (2^(c j - 1)), the first that does (2^(c j - 1) + 1), and their
    negatives"""
    e = [0, 1, R - 1, (R - 1) // 2, (R + 1) // 2, (1 << 32) - 1, 1 << 32, R - (1 << 32), 1 << 253]
    for j in range(1, FR_BITS // c + 1):
        for v in ((1 << (c * j)) - 1, 1 << (c * j - 1), (1 << (c * j - 1)) + 1):
            e += [v, R - v]
    return [v % R for v in e]
