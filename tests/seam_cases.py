"""Group-local inputs and references for the graph family at the sizes where its host drivers split work (no GPU, no library: numpy, the oracle and
the family's references in tests/refine_cases.py, reverse_cases.py, descent_cases.py, gsearch_cases.py, gfilter_cases.py; device_outputs and
host_arrays at the end of the first part are the GPU tests' shared plumbing and import torch when called).

Those references loop over rows in Python and cannot run over 10^5 .. 10^7 lines.  They do not have to: the stored rows are cut into consecutive
GROUPS of P = 97 rows (the last one partial), and line r = start + j names only rows of its own group,

    start + (j + o_t) mod 97,   t < in_k,   o_t = OFFSETS[t] (fixed, distinct, non-zero)

so N'(x), In(x), R'(x), C(a), every round of descent and every beam walk seeded inside a group stay inside that group, and the family's answer on
the lines of a group is the existing reference's answer on the 97-row sub-table, ids rebased (and the pair hash of R' taken of the absolute rows:
reverse_cases' row0).  97 is prime and divides none of the sizes at which a driver cuts (SEAMS) nor a difference of two of them, so a group
straddles every seam and a read displaced by a seam lands on another position of another group.  A line of the partial last group names rows past
the table through the mod 97: the out-of-range rule for free.

Irregularities, all inside groups: removed() takes the rows s - 1, s, s + 1 around every seam position s and two rows of every 13th group;
adversarial() gives a few lines of chosen groups refine_cases' adversarial forms (count 0, an all-ones entry, a repeated entry, an entry naming a
removed row, a self loop).  tests/test_seam_reference.py pins every local reference against the whole-table one on 5 x 97 + 40 rows."""
import numpy as np

from oracle import zebra_oracle as zo
from tests import gfilter_cases as gf
from tests import gsearch_cases as gc
from tests import refine_cases as rc
from tests import reverse_cases as rv

NONE = rc.NONE
P = 97
ID_BASE = 2**40 + 3
# the sizes at which the family's host drivers cut their work, as the GPU tests use them (tests/test_seam_reference.py parses the library's)
REFINE_SLAB = 65536        # ZH_REFINE_SLAB: stored rows of a sub-slab
HOST_ENTRIES = 2**25       # entries of a host entry's staged piece: refine_host_slab(k) = max(REFINE_SLAB, HOST_ENTRIES / k in whole sub-slabs)
GRAPH_BATCH = 16384        # ZH_GRAPH_BATCH: queries of one search launch
LINES_PER_LAUNCH = 2**24   # ZH_LINES_PER_LAUNCH: lines of one launch of a wave-per-line kernel
CSR_ENTRIES = 2**30        # entries of one launch of the transposition's edge passes
REFINE_CHUNK_BYTES = 64 << 20  # refine_chunk_bytes(): bytes of a host graph's u64 ids that one pinned chunk holds (8 388 608 entries)
SENTINEL = 0x5A5A5A5A      # what the tests fill a device output with before a call
SEAMS = (REFINE_SLAB, HOST_ENTRIES // 64, GRAPH_BATCH, LINES_PER_LAUNCH)
OFFSETS = tuple(int(o) for o in np.random.default_rng(0x5EA35).permutation(P - 1) + 1)  # a fixed order of 1 .. 96


def host_piece(k):
    """refine_host_slab(k): the lines of one staged piece of a host entry's output"""
    return max(REFINE_SLAB, HOST_ENTRIES // k // REFINE_SLAB * REFINE_SLAB)


def reverse_piece(rev_k):
    """the lines of one staged piece of zh_knn_graph_reverse's host entry"""
    return max(REFINE_SLAB, HOST_ENTRIES // rev_k)


def line_launches(n):
    """zh_line_launches(n)"""
    return -(-n // LINES_PER_LAUNCH)


def sub_slabs(first_row, n, live, piece=None):
    """the sub-slabs with a live line that a refinement over [first_row, first_row + n) launches: per piece of `piece` lines (a host entry's; None:
    the whole slab, a device entry's) every REFINE_SLAB rows from the piece's first row"""
    piece = n if piece is None else piece
    count = 0
    for p0 in range(first_row, first_row + n, piece):
        p1 = min(p0 + piece, first_row + n)
        count += sum(1 for r0 in range(p0, p1, REFINE_SLAB) if live[r0:min(r0 + REFINE_SLAB, p1)].any())
    return count


def descent_launches(n, live, in_k, rev_k, k, rounds_run, host):
    """zh_knn_graph_descent's `launches` for rounds > 1, term by term as descent_call (zh_api.hip) adds them up.  Only round 1's sub-slabs, its
    launch per piece and the host entry's emission per piece are counted where they are launched; the transposition's, the selection's and the
    flag / plan / emit terms come from the library's formula in n, so that asserting them shows no more than that n is past the cut"""
    piece = min(n, host_piece(k))
    pieces = -(-n // piece)
    csr = lambda w: 4 + 2 * (-(-n * w // CSR_ENTRIES))  # noqa: E731  (reverse_csr_launches)
    select = line_launches(n) + 1
    w = k + rev_k
    total = (select + csr(in_k) if rev_k else 0) + sub_slabs(0, n, live, piece) + pieces  # round 1
    total += (rounds_run - 1) * ((select + csr(k) if rev_k else 0) + 2 * line_launches(n) + (2 if w + w * w > 2048 else 1))
    return total + (pieces if host else line_launches(n))


def device_outputs(n, k, second=None):
    """sentinel-filled outputs of a device entry as torch tensors (torch is imported here: only the GPU tests call this): [n, k] i64, then
    [n, k] i64 and [n] i32 -- or, with second = "degree", [n] i32 twice (zh_knn_graph_reverse_device)"""
    import torch
    mid = torch.full((n, k), SENTINEL, dtype=torch.int64, device="cuda") if second is None else torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    return [torch.full((n, k), SENTINEL, dtype=torch.int64, device="cuda"), mid, torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")]


def host_arrays(out, lo=0, hi=None):
    """device_outputs' tensors, rows [lo, hi), on the host as the library's unsigned types"""
    return tuple(o[lo:hi].cpu().numpy().view(np.uint64 if o.dtype.itemsize == 8 else np.uint32) for o in out)


# ---------------------------------------------------------------------------------------------------------------- groups
def groups(n):
    return -(-n // P)


def span(g, n):
    """[start, end) of group g in a table of n rows"""
    return g * P, min(g * P + P, n)


def graph(n, in_k, id_base, lo=0, hi=None, group=P):
    """the lines [lo, hi) of the group-local graph over n stored rows: (ids [hi - lo, in_k] u64, counts [hi - lo] u32).  group: rows of a group
    where it is not 97 (the 128-row clusters of tests/test_gpu_large_table.py; OFFSETS stay below 97)"""
    hi = n if hi is None else hi
    r = np.arange(lo, hi, dtype=np.int64)[:, None]
    o = np.array(OFFSETS[:in_k], np.int64)[None, :]
    ids = r - r % group + (r % group + o) % group
    return ids.astype(np.uint64) + np.uint64(id_base), np.full(hi - lo, in_k, np.uint32)


def template(in_k):
    """C(j) of a fully live, regular group, per position j: the ascending positions (j + o_a) and (j + o_a + o_b) mod 97, j itself taken out"""
    o = np.array(OFFSETS[:in_k], np.int64)
    two = (o[:, None] + o[None, :]).reshape(-1)
    out = []
    for j in range(P):
        c = np.unique((j + np.concatenate([o, two])) % P)
        out.append(c[c != j])
    return out


def removed(n, positions):
    """the rows a test removes before any call: s - 1, s, s + 1 around every position s inside the table, and two rows of every 13th group, at
    places that change from group to group"""
    rows = {r for s in positions for r in (s - 1, s, s + 1) if 0 <= r < n}
    for g in range(5, groups(n), 13):
        a, b = (g * 7 + 3) % P, (g * 31 + 50) % P
        if a == b:
            b = (b + 1) % P
        rows |= {r for r in (g * P + a, g * P + b) if r < n}
    return np.array(sorted(rows), np.int64)


def seam_groups(n, positions):
    """the groups that straddle or touch a position: those of rows s - 1 and s"""
    return sorted({r // P for s in positions for r in (s - 1, s) if 0 <= r < n})


ADVERSARIAL_LINES = (3, 11, 23, 37, 52)  # positions inside a group: count 0, all-ones entry, repeated entry, removed row named, self loop


def adversarial(ids, counts, n, id_base, live, which, lo=0):
    """in place, for the lines [lo, lo + len(ids)) of graph(): the five forms on the lines ADVERSARIAL_LINES of every group of `which` (lines past
    the arrays or the table are left alone) -> the rows of the lines that were changed"""
    in_k = ids.shape[1]
    done = []
    for g in which:
        start, end = span(g, n)
        dead = np.flatnonzero(~live[start:end])
        for form, j in enumerate(ADVERSARIAL_LINES):
            r = start + j
            if not (lo <= r < lo + ids.shape[0] and r < n):
                continue
            i = r - lo
            if form == 0:
                counts[i] = 0
            elif form == 1:
                ids[i, 0] = NONE
            elif form == 2 and in_k >= 2:
                ids[i, in_k - 1] = ids[i, 0]
            elif form == 3 and dead.size:
                ids[i, 0] = np.uint64(id_base) + np.uint64(start + int(dead[0]))
            elif form == 4:
                ids[i, 0] = np.uint64(id_base) + np.uint64(r)
            else:
                continue
            done.append(r)
    return done


def checked_groups(n, positions, gone, changed, extra=32, seed=0x5EA36):
    """the groups check (a) takes: those at every position, the first and the last, every group with a removed or adversarial line, and `extra`
    further ones drawn by a fixed seed"""
    must = set(seam_groups(n, positions)) | {0, groups(n) - 1} | {int(r) // P for r in gone} | {int(r) // P for r in changed}
    rest = np.array(sorted(set(range(groups(n))) - must), np.int64)
    pick = np.random.default_rng(seed).permutation(rest.size)[:extra]
    return sorted(must | set(rest[pick].tolist()))


# ---------------------------------------------------------------------------------------------------------------- a table and its groups
class Table:
    """n synthetic rows of dimension d (zo.synth_rows, regenerated group by group, never held whole), ids id_base + row, the rows `gone` removed"""

    def __init__(self, n, d, id_base, gone=(), kind=0, seed=zo.SEED_ROWS, group=P):
        self.n, self.d, self.id_base, self.kind, self.seed, self.group = n, d, id_base, kind, seed, group
        self.gone = np.asarray(gone, np.int64)
        self.live = np.ones(n, bool)
        self.live[self.gone] = False
        self._rows = {}

    def span(self, g):
        return g * self.group, min((g + 1) * self.group, self.n)

    def rows(self, g):
        if g not in self._rows:
            s, e = self.span(g)
            self._rows[g] = zo.synth_rows(e - s, self.d, seed=self.seed, row0=s, kind=self.kind)
        return self._rows[g]

    def local(self, ids, counts, g):
        """the lines of group g (ids [rows of g, in_k] in the table's id space, counts) as a graph over the sub-table: row numbers from 0, id base 0;
        an entry that is no stored row stays out of range (2^64-1).  An entry naming a row of another group is a bug of the test"""
        s, e = self.span(g)
        ids = np.ascontiguousarray(ids, np.uint64)
        assert ids.shape[0] == e - s and len(counts) == e - s, (g, ids.shape, e - s)
        r = ids - np.uint64(self.id_base)
        stored = r < np.uint64(self.n)
        assert ((r[stored] >= np.uint64(s)) & (r[stored] < np.uint64(e))).all(), "group %d names a row of another group" % g
        out = np.full(ids.shape, NONE, np.uint64)
        out[stored] = r[stored] - np.uint64(s)
        return out, np.ascontiguousarray(counts, np.uint32)

    def rebase(self, ids, g):
        """a local answer's ids in the table's id space"""
        ids = ids.copy()
        ids[ids != NONE] += np.uint64(self.id_base + self.span(g)[0])
        return ids


# ---------------------------------------------------------------------------------------------------------------- the local references
def local_refine(tb, ids, counts, g, k, om, omode, rev_k=0):
    """zh_knn_graph_refine (rev_k = 0) or zh_knn_graph_refine_rev on the lines of group g -> (ids, keys, counts), the group's share of the info"""
    s, e = tb.span(g)
    lg = tb.local(ids, counts, g)
    in_k = lg[0].shape[1]
    if rev_k:
        (i, ky, c), info = rv.reference_rev(tb.rows(g), lg, in_k, rev_k, k, tb.live[s:e], 0, om, omode, row0=s)
    else:
        (i, ky, c), info = rc.reference(tb.rows(g), lg, in_k, k, tb.live[s:e], 0, om, omode)
    return (tb.rebase(i, g), ky, c), info


def local_reverse(tb, ids, counts, g, rev_k):
    """zh_knn_graph_reverse on the lines of group g -> (ids, counts, degree), the group's share of the info"""
    s, e = tb.span(g)
    lg = tb.local(ids, counts, g)
    (i, c, deg), info = rv.reference_reverse(lg, lg[0].shape[1], rev_k, tb.live[s:e], 0, row0=s)
    return (tb.rebase(i, g), c, deg), info


def local_descent(tb, ids, counts, g, rev_k, k, rounds_run, om, omode):
    """zh_knn_graph_descent on the lines of group g after rounds_run rounds (the CALL's count: a group that stops changing earlier is at a fixed
    point, and the loop here just goes on) -> (ids, keys, counts)"""
    s, e = tb.span(g)
    graph_, live = tb.local(ids, counts, g), tb.live[s:e]
    w = graph_[0].shape[1]
    K = rc.key_rows(tb.rows(g), om, omode, np.flatnonzero(live).tolist())
    for _ in range(rounds_run):
        (i, ky, c), _info = rv.reference_rev(tb.rows(g), graph_, w, rev_k, k, live, 0, om, omode, K=K, row0=s)
        graph_, w = (i, c), k
    return tb.rebase(i, g), ky, c


def local_seeds(tb, seeds, g):
    """seed ids of the table's id space as ids over group g's sub-table (id base 0); a seed that is no row of the group becomes 2^64-1"""
    s, e = tb.span(g)
    r = np.asarray(seeds, np.uint64) - np.uint64(tb.id_base)
    ok = (r >= np.uint64(s)) & (r < np.uint64(e))
    out = np.full(r.shape, NONE, np.uint64)
    out[ok] = r[ok] - np.uint64(s)
    return out


def local_search(tb, ids, counts, g, Q, seeds, top_k, beam, width, max_iters, om, omode, allowed=None):
    """zh_search_graph_batch for queries whose valid seeds all lie in group g, the attached graph being the table's whole graph (ids, counts: the
    group's lines) -> (ids, keys, counts), info.  allowed: a mask over ALL stored rows -- zh_search_graph_filtered_batch"""
    s, e = tb.span(g)
    lg = tb.local(ids, counts, g)
    sd = local_seeds(tb, seeds, g)
    args = (tb.rows(g), lg, e - s, lg[0].shape[1], tb.live[s:e], 0, Q, sd, top_k, beam, width, max_iters, om, omode)
    if allowed is None:
        (i, ky, c), info = gc.reference(*args)
    else:
        words, n_bits = gf.bitmap(np.asarray(allowed, bool)[s:e])
        (i, ky, c), info = gf.reference(*args, words, n_bits)
    return (tb.rebase(i, g), ky, c), info
