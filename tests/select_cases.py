"""Case builders and plain references for tests/test_select_stress.py: the kernels that turn RPN outputs into proposal lists
(csrc/nms.hip, csrc/proposals.hip).  CPU only, imports without a GPU.

NMS cases are constructed suppression graphs.  Boxes live in disjoint cells: cell c is [32 c, 32 c + 16] x [0, h] with the three
nested heights 16 / 12 / 9 (kinds A / B / C), so IoU(A, B) = IoU(B, C) = 3/4, IoU(A, C) = 9/16, boxes of one kind in one cell
have IoU 1 and boxes of different cells never overlap.  Every coordinate is an integer below 2^24: areas, intersections and
the three quotients are exact in fp32 and far from the 0.7 threshold.  A case is a row count plus a plan
{row: (earlier row whose cell it shares, kind)}; every unplanned row is an A box alone in a fresh cell.  The reference is the
definition (strict >, only kept rows suppress, cut at max_keep) evaluated per cell with fractions.Fraction: O(M), usable at
the 32,768 rows where the dense oracle (an M x M matrix) is not.

What the scan kernel's bookkeeping is driven with, by name (a "chunk" is 64 rows, c = row >> 6, bit = row & 63):
  * a suppressor in chunk c and its victim in chunk c + d: d = 0 is the diagonal word, 1 and 2 the prefetched near words,
    >= 3 the far words, whose removed word c + d lives in lane (c + d) & 63, slot (c + d) >> 6;
  * the suppressor's rank among the kept rows of its chunk: the far words of the first 16 kept rows (nms_scan_kernel<3, 2>;
    the wide instantiation defers 8) are loaded into one of two register sets (c even / c odd) and merged a chunk later,
    those of further kept rows at once.  Classes here: 'def' rank < 8 (deferred in both instantiations), 'mid' 8 <= rank < 16
    (deferred in <3, 2> only), 'imm' rank >= 16 (immediate in both).

Top-k, merge, decode and gather cases are plain tensors (torch, CPU); the test moves them to the device and compares with the
tensor expressions there.
"""
import functools
import math
from collections import Counter
from fractions import Fraction

import numpy as np
import torch

CHUNK = 64
KIND_HEIGHT = {'A': 16, 'B': 12, 'C': 9}
VICTIM_BITS = (0, 31, 32, 63)
FAR_DISTANCES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191)
WIDE_DISTANCES = (192, 255, 256, 511)
NARROW_SIZES = (4497, 12000, 12288)          # nms_scan_kernel<3, 2>
WIDE_SIZES = (12289, 16385, 32768)           # nms_scan_kernel<MAX_WORDS_PER_LANE, 1>
NMS_MAX_ROWS = 32768
SCAN_NARROW, SCAN_WIDE = 'nms_scan_kernel<3, 2>', 'nms_scan_kernel<MAX_WORDS_PER_LANE, 1>'
RANK_CLASS = {'def': (0, 8), 'mid': (8, 16), 'imm': (16, 64)}
# suppressor bits per class: never a victim bit; at most one victim bit (0) lies below 16, so rank >= bit - 1
_SUP_BITS = {'def': tuple(range(1, 8)), 'mid': tuple(range(9, 16)), 'imm': tuple(range(17, 31)) + tuple(range(33, 63)),
             'any': tuple(b for b in range(1, 63) if b not in (31, 32))}
NMS_FAMILIES = ('disjoint', 'far', 'first_needed', 'chain', 'sparse', 'cut', 'strict')
PLANTED_SCANS = ('suppressed_suppress', 'drop_far', 'drop_dist3', 'first16_far', 'first8_far', 'ge', 'past_counts')


def scan_name(M):
    """the scan instantiation the launcher picks for M rows per image, as tests/infer_audit.py names it"""
    words = (M + 63) // 64
    return SCAN_NARROW if words <= 64 * 3 else SCAN_WIDE


def _iou(ka, kb):
    a, b = KIND_HEIGHT[ka], KIND_HEIGHT[kb]
    return Fraction(min(a, b), max(a, b))


class NmsCase:
    """M rows, plan {row: (earlier row, kind)}, max_keep (<= 0: all), fp32 threshold, count = valid rows (the rest is
    there to be ignored)"""

    def __init__(self, name, M, plan, max_keep=-1, thr=0.7, count=None, pairs=(), chains=()):
        assert 1 <= M <= NMS_MAX_ROWS
        self.name, self.M, self.plan, self.max_keep = name, M, dict(plan), int(max_keep)
        self.thr = np.float32(thr)
        self.count = M if count is None else int(count)
        self.pairs, self.chains = list(pairs), list(chains)
        rows = np.fromiter(sorted(self.plan), np.int64, len(self.plan))
        fresh = np.ones(M, np.int64)
        fresh[rows] = 0
        cell = np.cumsum(fresh) - 1
        kind = np.full(M, 'A', dtype='<U1')
        for r in rows:
            e, k = self.plan[int(r)]
            assert 0 <= e < r < M and k in KIND_HEIGHT, (name, r, e, k)
            cell[r] = cell[e]
            kind[r] = k
        self.cell, self.kind = cell, kind
        shared = np.zeros(M, bool)
        shared[rows] = True
        shared[[self.plan[int(r)][0] for r in rows]] = True
        self.shared_rows = np.nonzero(shared)[0]

    def with_(self, name, **kw):
        args = dict(max_keep=self.max_keep, thr=self.thr, count=self.count, pairs=self.pairs, chains=self.chains)
        args.update(kw)
        return NmsCase(name, self.M, self.plan, **args)

    def boxes(self):
        """[M, 4] fp32 (x1, y1, x2, y2); every coordinate an integer below 2^24"""
        x1 = 32 * self.cell
        h = np.array([KIND_HEIGHT[k] for k in 'ABC'])[np.searchsorted(np.array(list('ABC')), self.kind)]
        b = np.stack([x1, np.zeros_like(x1), x1 + 16, h], 1)
        assert b.max() < 2 ** 24 and b.min() >= 0
        out = b.astype(np.float32)
        assert np.array_equal(out.astype(np.int64), b)
        return out

    def _cut(self, kept_flags, n):
        keep = np.nonzero(kept_flags[:n])[0].astype(np.int64)
        return keep[:self.max_keep] if 0 < self.max_keep < len(keep) else keep

    @functools.lru_cache(maxsize=None)
    def kept_flags(self):
        """the definition, cell by cell: a row is suppressed when a KEPT earlier row of its cell has IoU > thr with it"""
        thr = Fraction(float(self.thr))
        kept = np.ones(self.M, bool)
        by_cell = {}
        for r in self.shared_rows:
            by_cell.setdefault(int(self.cell[r]), []).append(int(r))
        for rows in by_cell.values():
            alive = []
            for r in rows:                       # ascending
                if any(_iou(self.kind[e], self.kind[r]) > thr for e in alive):
                    kept[r] = False
                else:
                    alive.append(r)
        return kept

    def expected(self):
        """the keep list: ascending indices of the kept rows among the first `count`, cut at max_keep"""
        return self._cut(self.kept_flags(), self.count)

    def kept_rank(self, row):
        """rank of `row` among the kept rows of its 64-row chunk"""
        return int(self.kept_flags()[row // CHUNK * CHUNK:row].sum())


def planted_scan(case, bug=None):
    """One greedy scan in row order with a planted error (None: the correct scan, a second statement of the reference):
    suppressed_suppress  a suppressed row still suppresses
    drop_far             hits at chunk distance >= 3 are lost
    drop_dist3           hits at chunk distance exactly 3 are lost (the deferred words merged a chunk late)
    first16_far          only the first 16 kept rows of a chunk carry their far hits
    first8_far           only the first 8 do (the wide instantiation defers one round of 8)
    ge                   IoU >= thr suppresses
    past_counts          rows past `count` are walked (their mask words were never computed: nothing suppresses them)"""
    assert bug is None or bug in PLANTED_SCANS
    thr = Fraction(float(case.thr))
    kept = np.ones(case.M, bool)
    seen = {}
    for r in case.shared_rows:
        r = int(r)
        if r >= case.count:
            continue
        members = seen.setdefault(int(case.cell[r]), [])
        for e in members:
            if not (kept[e] or bug == 'suppressed_suppress'):
                continue
            v = _iou(case.kind[e], case.kind[r])
            hit = v >= thr if bug == 'ge' else v > thr
            d = r // CHUNK - e // CHUNK
            if (bug == 'drop_far' and d >= 3) or (bug == 'drop_dist3' and d == 3):
                hit = False
            if bug in ('first16_far', 'first8_far') and d >= 3 and \
                    kept[e // CHUNK * CHUNK:e].sum() >= (16 if bug == 'first16_far' else 8):
                hit = False
            if hit:
                kept[r] = False
                break
        members.append(r)
    return case._cut(kept, case.M if bug == 'past_counts' else case.count)


class _Planner:
    """places suppressor / victim pairs and chains on free rows; _finish() asserts on the reference that every planted row
    has the chunk, bit and kept-rank it was meant to have"""

    def __init__(self, M, keepers_per_chunk=None):
        self.M, self.nchunks = M, (M + CHUNK - 1) // CHUNK
        self.plan, self.role, self.pairs, self.chains = {}, {}, [], []
        self.keepers, self.limit = Counter(), keepers_per_chunk

    def free(self, row, keeper=False):
        if not (0 <= row < self.M) or row in self.role:
            return False
        return not (keeper and self.limit is not None and self.keepers[row // CHUNK] >= self.limit)

    def take(self, row, role):
        assert self.free(row, role != 'drop'), row
        self.role[row] = role
        if role != 'drop':
            self.keepers[row // CHUNK] += 1

    def _chunks(self, parity, last):
        start = (37 * (len(self.pairs) + len(self.chains))) % self.nchunks
        for i in range(self.nchunks):
            c = (start + i) % self.nchunks
            if c % 2 == parity and c <= last:
                yield c

    def pair(self, d, vbit, cls, parity, kind='B', chunk=None):
        """an A suppressor of rank class `cls` in a chunk c of the given parity, its victim at bit vbit of chunk c + d"""
        for c in ([chunk] if chunk is not None else self._chunks(parity, self.nchunks - 1 - d)):
            v = (c + d) * CHUNK + vbit
            if not self.free(v):
                continue
            for b in _SUP_BITS[cls]:
                s = c * CHUNK + b
                if s < v and self.free(s, True):
                    self.take(s, 'keep')
                    self.take(v, 'drop')
                    self.plan[v] = (s, kind)
                    self.pairs.append(dict(sup=s, victim=v, d=d, bit=vbit, cls=cls, parity=parity, kind=kind))
                    return True
        return False

    def chain(self, dab, dbc, parity, bits=(5, 40, 50)):
        """A -> B -> C in one cell: A kept, B suppressed by A, C (IoU 9/16 with A) must survive"""
        for c in self._chunks(parity, self.nchunks - 1 - dab - dbc):
            rows, prev = [], -1
            for ch, b0 in zip((c, c + dab, c + dab + dbc), bits):
                r = next((ch * CHUNK + b for b in list(range(b0, 63)) + list(range(1, b0))
                          if ch * CHUNK + b > prev and ch * CHUNK + b not in rows and b not in VICTIM_BITS
                          and self.free(ch * CHUNK + b, True)), None)
                if r is None:
                    break
                rows.append(r)
                prev = r
            if len(rows) == 3:
                a, b, cc = rows
                self.take(a, 'keep'), self.take(b, 'drop'), self.take(cc, 'keep')
                self.plan[b], self.plan[cc] = (a, 'B'), (b, 'C')
                self.chains.append(dict(a=a, b=b, c=cc, dab=dab, dbc=dbc, parity=parity))
                return True
        return False

    def sparsify(self):
        """in-chunk duplicates: every chunk keeps 1 + (c % 8) rows at the most (planted keepers included)"""
        self.limit = None
        for c in range(self.nchunks):
            rows = [r for r in range(c * CHUNK, min(self.M, (c + 1) * CHUNK)) if r not in self.role]
            if not rows:
                continue
            base, rest = rows[0], rows[1:]
            extra = max(0, 1 + (c % 8) - self.keepers[c] - 1)
            step = max(1, len(rest) // (extra + 1))
            stay = set(rest[step - 1::step][:extra])
            self.take(base, 'keep')
            for r in rest:
                if r in stay:
                    self.take(r, 'keep')
                else:
                    self.take(r, 'drop')
                    self.plan[r] = (base, 'A')

    def finish(self, name, **kw):
        case = NmsCase(name, self.M, self.plan, pairs=self.pairs, chains=self.chains, **kw)
        check_planted(case)
        return case


def check_planted(case):
    """the preconditions of a constructed case, on its reference (at the 0.7 threshold's graph: A/B and B/C suppress)"""
    kept = case.kept_flags()
    strict = Fraction(float(case.thr)) >= Fraction(3, 4)
    for p in case.pairs:
        s, v = p['sup'], p['victim']
        assert kept[s] and (kept[v] if strict and p['kind'] == 'B' else not kept[v]), (case.name, p)
        assert v // CHUNK - s // CHUNK == p['d'] and v % CHUNK == p['bit'] and (s // CHUNK) % 2 == p['parity'], (case.name, p)
        lo, hi = RANK_CLASS[p['cls']] if p['cls'] in RANK_CLASS else (0, 8)
        assert lo <= case.kept_rank(s) < hi, (case.name, p, case.kept_rank(s))
    for ch in case.chains:
        a, b, c = ch['a'], ch['b'], ch['c']
        assert kept[a] and kept[c] and (kept[b] if strict else not kept[b]), (case.name, ch)
        assert b // CHUNK - a // CHUNK == ch['dab'] and c // CHUNK - b // CHUNK == ch['dbc'], (case.name, ch)


def _distances(M):
    nchunks = (M + CHUNK - 1) // CHUNK
    ds = FAR_DISTANCES + (WIDE_DISTANCES if scan_name(M) == SCAN_WIDE else ())
    return [d for d in ds if d <= nchunks - 1]


def _plant_far(p, classes=('def', 'imm'), optional=('def', 'mid', 'imm')):
    """every distance that fits x {deferred, immediate} x {c even, c odd} is REQUIRED, with the victim bits cycling; the
    rest of the product distance x bit x rank class x parity is planted where free rows remain"""
    n = 0
    for d in sorted(_distances(p.M), reverse=True):          # the most constrained first
        for cls in classes:
            for parity in (0, 1):
                bits = [b for b in VICTIM_BITS if not (d == 0 and b == 0)]
                order = bits[n % len(bits):] + bits[:n % len(bits)]
                if not any(p.pair(d, b, cls, parity) for b in order):
                    # only where no victim row is left (d reaches the last, partial chunk; c = 0 alone is possible)
                    assert not [1 for c in range(parity, p.nchunks - d, 2) for b in bits if p.free((c + d) * CHUNK + b)], \
                        (p.M, d, cls, parity)
                n += 1
    for d in _distances(p.M):
        for cls in optional:
            for parity in (0, 1):
                for b in VICTIM_BITS:
                    have = any((q['d'], q['cls'], q['parity'], q['bit']) == (d, cls, parity, b) for q in p.pairs)
                    if not have and not (d == 0 and b == 0):
                        p.pair(d, b, cls, parity)
    assert {q['bit'] for q in p.pairs} == set(VICTIM_BITS)


def _plant_chains(p):
    for dab in (0, 1, 2, 3, 7):
        for dbc in (0, 1, 3, 6):
            for parity in (0, 1):
                assert p.chain(dab, dbc, parity), (p.M, dab, dbc, parity)


def _plant_first_needed(p):
    """the suppressor is the last kept row of chunk c (bit 63), the victim bit 0 of chunk c + 3: the earliest row the far
    words serve.  Once with 7 kept rows in chunk c (deferred words), once with all 64 (immediate), c even and odd, early and
    at the end of the image."""
    last = p.nchunks - 1
    ce, co = (last - 3) - (last - 3) % 2, (last - 3) - (last - 2) % 2          # the last even / odd chunk with c + 3 <= last
    chunks = {'def': (2, 7, ce, co), 'imm': (12, 17, ce - 8, co - 8)}
    for cls, cs in chunks.items():
        assert {c % 2 for c in cs} == {0, 1}
        for c in sorted(set(cs)):
            assert 0 <= c and c + 3 <= last, (p.M, c)
            s, v = c * CHUNK + 63, (c + 3) * CHUNK
            p.take(s, 'keep'), p.take(v, 'drop')
            p.plan[v] = (s, 'B')
            if cls == 'def':
                for b in range(0, 6):
                    p.take(c * CHUNK + b, 'keep')
                for b in range(6, 63):
                    p.take(c * CHUNK + b, 'drop')
                    p.plan[c * CHUNK + b] = (c * CHUNK, 'A')
            p.pairs.append(dict(sup=s, victim=v, d=3, bit=0, cls='def' if cls == 'def' else 'imm', parity=c % 2, kind='B'))


@functools.lru_cache(maxsize=None)
def nms_family(name, M):
    """the cases of one named family at M rows"""
    if name == 'disjoint':
        return [NmsCase(f'disjoint/{M}/keep{k}', M, {}, max_keep=k) for k in (-1, 1, 64, 65, 1000, M, M + 5)]
    if name == 'far':
        p = _Planner(M)
        _plant_far(p)
        return [p.finish(f'far/{M}')]
    if name == 'first_needed':
        p = _Planner(M)
        _plant_first_needed(p)
        case = p.finish(f'first_needed/{M}')
        for q in case.pairs:                      # the last kept row of its chunk
            assert q['sup'] % CHUNK == 63 and case.kept_flags()[q['sup']]
        return [case]
    if name == 'chain':
        p = _Planner(M)
        _plant_chains(p)
        return [p.finish(f'chain/{M}')]
    if name == 'sparse':
        p = _Planner(M, keepers_per_chunk=4)
        _plant_far(p, classes=('any',), optional=())
        for dab, dbc in ((0, 0), (1, 3), (3, 1), (7, 6), (2, 0)):
            assert p.chain(dab, dbc, (dab + dbc) % 2)
        p.sparsify()
        case = p.finish(f'sparse/{M}')
        per_chunk = np.add.reduceat(case.kept_flags().astype(np.int64), np.arange(0, M, CHUNK))[:M // CHUNK]     # full chunks
        assert per_chunk.min() >= 1 and per_chunk.max() <= 8, (per_chunk.min(), per_chunk.max())
        assert len(set(per_chunk.tolist())) >= 6
        return [case]
    if name == 'cut':
        base = nms_family('far', M)[0]
        full = base.expected()
        kept = base.kept_flags()
        sups = sorted(q['sup'] for q in base.pairs if q['d'] >= 3 and q['sup'] % CHUNK < 50)
        picks = [sups[len(sups) // 2], next(s for s in sups[len(sups) // 3:] if (s // CHUNK) % 2 == 1),
                 next(s for s in sups if (s // CHUNK) % 2 == 0 and s // CHUNK >= 2)]
        out = []
        for s in picks:
            for more in (1, 3):                  # the cut lands on the suppressor / two kept rows after it
                k = int(np.searchsorted(full, s)) + more
                case = base.with_(f'cut/{M}/keep{k}', max_keep=k)
                last = int(case.expected()[-1])
                assert np.array_equal(case.expected(), full[:k]) and len(case.expected()) == k
                assert last // CHUNK == s // CHUNK and kept[last + 1:(last // CHUNK + 1) * CHUNK].any()   # mid-chunk
                out.append(case)
        return out
    if name == 'strict':
        p = _Planner(M)
        last = p.nchunks - 1
        n = 0
        for d in (0, 3, 4, min(64, last - 2), last - 2):
            for cls in ('def', 'imm'):
                for parity in (0, 1):
                    if d == 0:                  # victims in chunk 0
                        ok = parity == 1 or p.pair(0, (31, 32, 63)[n % 3], cls, 0, chunk=0)
                    else:
                        ok = any(p.pair(d, VICTIM_BITS[(n + i) % 4], cls, parity) for i in range(4))
                    assert ok, (M, d, cls, parity)
                    n += 1
        below = np.nextafter(np.float32(0.75), np.float32(0))
        at, under = p.finish(f'strict/{M}/at', thr=0.75), p.finish(f'strict/{M}/below', thr=below)
        assert Fraction(float(at.thr)) == Fraction(192, 256) and Fraction(float(under.thr)) < Fraction(192, 256)
        vs = [q['victim'] for q in at.pairs]
        assert at.kept_flags()[vs].all() and not under.kept_flags()[vs].any()
        assert any(v < CHUNK for v in vs) and any(q['d'] >= 3 for q in at.pairs)
        return [at, under]
    raise KeyError(name)


def counts_cases(Mmax):
    """four images of one launch with counts (0, 1, Mmax, Mmax - 63): the `far` graph, rows past each count overwritten
    with copies of row 0.  Returns (boxes [4, Mmax, 4], counts, cases)."""
    base = nms_family('far', Mmax)[0]
    counts = (0, 1, Mmax, Mmax - 63)
    boxes, cases = [], []
    for n in counts:
        b = base.boxes().copy()
        b[n:] = b[0]
        boxes.append(b)
        cases.append(base.with_(f'counts/{Mmax}/{n}', count=n))
    return np.stack(boxes), counts, cases


# ======================================================================================================= top-k rows
class TopkCase:
    """levels: one [I, A, H, W] fp32 logit tensor per level; the row of image i is the level in (h, w, a) order"""

    def __init__(self, name, levels, nms_pre):
        self.name, self.levels, self.nms_pre = name, levels, int(nms_pre)

    @property
    def dims(self):
        return [(int(t.shape[2]), int(t.shape[3]), int(t.shape[1])) for t in self.levels]

    def rows(self, level=0):
        """[I, n] logits in the kernel's element order"""
        t = self.levels[level]
        return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)


def _level(rows, A=1):
    """[I, n] rows in (h, w, a) order -> [I, A, H, W]"""
    rows = torch.as_tensor(np.asarray(rows, np.float32))
    I, n = rows.shape
    assert n % A == 0
    pix = n // A
    H = next(h for h in range(int(math.isqrt(pix)), 0, -1) if pix % h == 0)
    return rows.reshape(I, H, pix // H, A).permute(0, 3, 1, 2).contiguous()


def _quantised(rng, shape, scale=3.0, step=0.25):
    """random logits on a coarse grid (exact in bf16): many exact ties"""
    return (np.round(rng.standard_normal(shape) * scale / step) * step).astype(np.float32)


def stable_topk(scores, k):
    """indices of the k largest in stable descending order"""
    return np.argsort(-scores.astype(np.float64), kind='stable')[:k]


def planted_topk(scores, k, bug):
    """'unstable': ties in DESCENDING index order; 'cut_last': the tie group cut by k keeps its last members"""
    n = len(scores)
    idx = np.arange(n)
    if bug == 'unstable':
        return np.lexsort((-idx, -scores.astype(np.float64)))[:k]
    assert bug == 'cut_last'
    if k >= n:
        return stable_topk(scores, k)
    T = scores[stable_topk(scores, k)[-1]]
    above, tie = idx[scores > T], idx[scores == T]
    sel = np.concatenate([above, tie[len(tie) - (k - len(above)):]])
    return sel[np.argsort(-scores[sel].astype(np.float64), kind='stable')]


def _straddle_rows(k=500, n=3 * 4096):
    """two logit values: the tie group of the larger one is cut by k, its last kept member is index 4095 in row 0 and 4096
    in row 1; rows 2 and 3 add 50 larger scores on both sides of the boundary"""
    rows = np.full((4, n), -2.0, np.float32)
    for r, (last, top) in enumerate(((4095, 0), (4096, 0), (4095, 50), (4096, 50))):
        need = k - top
        rows[r, last - need + 1:last + 1 + 300] = 1.5
        if top:
            pos = np.r_[np.arange(100, 100 + top // 2), np.arange(9000, 9000 + top - top // 2)]
            rows[r, pos] = 6.0
        keep = stable_topk(rows[r], k)
        T = rows[r][keep[-1]]
        tie = np.nonzero(rows[r] == T)[0]
        kept_tie = np.intersect1d(keep, tie)
        assert T == 1.5 and kept_tie.max() == last and len(tie) > len(kept_tie) == need      # cut inside the tie group
        assert tie.min() <= 4095 and tie.max() >= 4096                                         # which straddles the chunks
    return rows


@functools.lru_cache(maxsize=None)
def topk_cases():
    rng = np.random.default_rng(11)
    cases = []
    n = 3 * 4096 + 5
    eq = np.stack([np.full(n, 0.5, np.float32), np.full(n, -3.0, np.float32)])
    cases += [TopkCase('all_equal/k500', [_level(eq)], 500), TopkCase(f'all_equal/k{n - 1}', [_level(eq)], n - 1)]
    cases.append(TopkCase('straddle', [_level(_straddle_rows())], 500))
    for n in (4096, 4097, 8192):
        rows = _quantised(rng, (2, n))
        for k in (1, n - 1, n, n + 7):
            cases.append(TopkCase(f'edges/n{n}/k{k}', [_level(rows)], k))
    n, k = 5000, 500
    rows = _quantised(rng, (2, n))
    for r in range(2):
        pos = rng.permutation(n)[:700]
        rows[r, pos] = rng.choice(np.array([17.0, 18.0, 20.5, 30.0, 88.0, 100.0], np.float32), 700)
        assert (rows[r] >= 17).sum() > k
    cases.append(TopkCase('ones', [_level(rows)], k))
    rows = np.full((2, n), -200.0, np.float32)
    for r in range(2):
        pos = rng.permutation(n)[:300]
        rows[r, pos] = _quantised(rng, 300)
        assert (rows[r] > -200).sum() < k
    cases.append(TopkCase('zeros', [_level(rows)], k))
    n = 6000
    j = np.arange(n, dtype=np.float32)
    rows = np.stack([j[::-1], j, rng.permutation(j)]) * np.float32(2.0 ** -20)
    s = (1.0 / (1.0 + np.exp(-rows.astype(np.float32)))).astype(np.float32).view(np.uint32)
    assert len(np.unique(s >> 20)) == 1 and len(np.unique(s[0] >> 8)) * 8 < len(np.unique(s[0]))
    cases.append(TopkCase('low_bits', [_level(rows)], 500))
    dims = [(5, 7, 3), (3, 4, 3), (2, 3, 3), (2, 2, 3), (1, 2, 3), (1, 1, 3)]
    cases.append(TopkCase('rows48', [torch.as_tensor(_quantised(rng, (8, a, h, w))) for h, w, a in dims], 20))
    assert 8 * len(dims) == 48
    cases.append(TopkCase('k16384', [torch.as_tensor(_quantised(rng, (1, 5, 50, 80), scale=4.0, step=0.0625))], 16384))
    return cases


def tiny_case():
    """fp32 logits -104 ... -87 in steps of 1/64, three of each, shuffled: 1 / (1 + e^-x) is subnormal below -87.34 and 0
    once e^-x overflows"""
    rng = np.random.default_rng(12)
    v = -104.0 + np.arange(17 * 64 + 1, dtype=np.float32) / 64
    rows = np.stack([rng.permutation(np.repeat(v, 3)) for _ in range(2)])
    assert rows.min() == -104 and rows.max() == -87
    return TopkCase('tiny', [_level(rows, A=3)], 2000)


# ================================================================================================ merge / decode / gather
class MergeCase:
    """levels given directly: ks per level, scores [I, M] (every level stably descending), valid [I, M] uint8, props [I, M, 4]"""

    def __init__(self, name, ks, scores, valid, props):
        self.name, self.ks, self.scores, self.valid, self.props = name, list(ks), scores, valid, props


MERGE_SHAPES = {'five': (300, 200, 100, 50, 7), 'one': (1,), 'empty_level': (40, 0, 25), 'eight': (64, 33, 17, 9, 5, 3, 2, 1),
                'lds_limit': (9000, 6000, 3000, 1000, 199)}
MERGE_MAX_ROWS = 19199
VALID_MODES = ('half', 'all', 'none', 'one_image_clear')


def merge_case(shape, mode, n_img=3, seed=5):
    ks = MERGE_SHAPES[shape]
    M = sum(ks)
    assert M <= MERGE_MAX_ROWS
    g = torch.Generator().manual_seed(seed + M)
    # scores on a grid of 33 values: equal scores inside every level and across levels
    grid = max(4, min(32, M // 4))
    parts = [torch.randint(0, grid + 1, (n_img, k), generator=g).float().div(grid).sort(dim=1, descending=True, stable=True)[0]
             for k in ks]
    scores = torch.cat(parts, 1)
    if len([k for k in ks if k]) > 1 and M >= 8:
        for a, b in zip(parts[:-1], parts[1:]):
            if a.shape[1] >= 16 and b.shape[1] >= 16:
                assert len(np.intersect1d(a[0].numpy(), b[0].numpy())) > 0          # cross-level ties
    valid = {'half': torch.rand((n_img, M), generator=g) < 0.5, 'all': torch.ones((n_img, M), dtype=torch.bool),
             'none': torch.zeros((n_img, M), dtype=torch.bool)}.get(mode)
    if mode == 'one_image_clear':
        valid = torch.rand((n_img, M), generator=g) < 0.5
        valid[1] = False
    xy = torch.rand((n_img, M, 2), generator=g) * 700
    wh = torch.rand((n_img, M, 2), generator=g) * 300
    props = torch.cat([xy, xy + wh], 2)
    return MergeCase(f'{shape}/{mode}', ks, scores, valid.to(torch.uint8), props)


DECODE_MEANS, DECODE_STDS = (0.1, -0.2, 0.05, -0.05), (0.5, 0.5, 0.25, 0.25)
# the same means with stds that are no powers of two: d * std is rounded, so a fused multiply-add (or any other order of
# d * std + mean) changes bits, which the exact products of the set above cannot show
DECODE_OPERANDS = {'pow2': (DECODE_MEANS, DECODE_STDS), 'tenths': (DECODE_MEANS, (0.1, 0.1, 0.2, 0.2))}
MAX_RATIO = abs(math.log(16 / 1000))            # = log(1000 / 16)


def fma_differs(d, stds, means):
    """how many elements of fp32 d * std + mean change when the product is not rounded (fp64 holds it exactly)"""
    d32 = d.float()
    st, mn = torch.tensor(stds, dtype=torch.float32), torch.tensor(means, dtype=torch.float32)
    two = d32 * st + mn
    fused = (d32.double() * st.double() + mn.double()).float()
    return int((two != fused).sum())


def decode_case(operands='pow2', seed=7, n_img=3):
    """three levels of (deltas [I, 4 A, H, W], anchors [H W A, 4], index [I, k], scores [I, k]) + per-image (W, H) limits.
    Deltas are exact in bf16; d * std + mean reaches and passes +/- log(1000 / 16), centre shifts push boxes wholly outside
    the image."""
    means, stds = DECODE_OPERANDS[operands]
    g = torch.Generator().manual_seed(seed)
    levels = []
    for (H, W, A), stride, k in (((12, 17, 3), 8, 300), ((6, 9, 3), 16, 162), ((3, 5, 3), 32, 20)):
        n = H * W * A
        d = (torch.randn((n_img, n, 4), generator=g) * 2).mul(8).round().div(8)
        edge = torch.tensor([MAX_RATIO, -MAX_RATIO, MAX_RATIO * 1.5, -MAX_RATIO * 1.5, 40.0, -40.0])
        edge = ((edge - means[2]) / stds[2]).bfloat16().float()
        pick = torch.randint(0, len(edge), (n_img, n, 2), generator=g)
        hot = torch.rand((n_img, n, 2), generator=g) < 0.3
        d[..., 2:] = torch.where(hot, edge[pick], d[..., 2:])
        far = torch.rand((n_img, n, 2), generator=g) < 0.2
        d[..., :2] = torch.where(far, d[..., :2] * 16, d[..., :2])            # centres far outside the image
        assert torch.equal(d.bfloat16().float(), d)
        assert (fma_differs(d, stds, means) > 100) == (operands == 'tenths'), (operands, fma_differs(d, stds, means))
        deltas = d.reshape(n_img, H, W, A * 4).permute(0, 3, 1, 2).contiguous()
        cy, cx = torch.meshgrid(torch.arange(H) * stride, torch.arange(W) * stride, indexing='ij')
        ctr = torch.stack([cx, cy], -1).reshape(-1, 1, 2).float()
        half = torch.tensor([[stride * 4.0, stride * 2.0], [stride * 3.0, stride * 3.0], [stride * 2.0, stride * 4.0]])[None]
        anchors = torch.cat([ctr - half, ctr + half], -1).reshape(n, 4)
        index = torch.stack([torch.randperm(n, generator=g)[:k] for _ in range(n_img)])
        scores = torch.rand((n_img, k), generator=g).sort(dim=1, descending=True)[0]
        levels.append(dict(deltas=deltas, anchors=anchors, index=index, scores=scores, dims=(H, W, A), k=k))
    lim = torch.tensor([[136.0, 96.0], [100.0, 75.0], [61.0, 90.0]])[:n_img]
    return levels, lim
