"""The split rule both BVH builders share (bf_bvh.cpp: Builder::build, restated by bf_build.hip: eval_kernel), in numpy, as a
VERIFIER of finished trees: tests/bvh_tree_check.py says whether a tree is valid, this file says whether its splits are the binned-SAH
splits and whether the collapses adopted by the documented rule.

Input: what capi.Scene.read_bvh(4) returns (nodes, rows float32[n, 3, 4] in leaf order, root).  Rows are in leaf order, so every child
reference covers a contiguous slot range and a node's children tile its range (asserted).  A four-wide node holds at most four ranges
that came from a binary subtree: every way to cut the ranges, in slot order, into a left prefix and a right rest (recursively) is a
candidate grouping; a grouping is allowed if every binary node in it is allowed by the rule; a four-wide node passes if at least one
grouping is allowed, and its children take their binary depths from the allowed groupings (the root is at depth 0).

The rule for a binary node of `count` triangles at depth `depth` with `mid` of them on the left (count > kMaxLeaf, else it is a leaf):
  forced      need = the smallest k with kMaxLeaf << k >= count; if depth + need + 1 >= kMaxDepth (31): mid == count // 2
  coincident  no axis has a float32 centroid extent above 0: mid == count // 2
  sah         centroids 0.5f (lo + hi) of the triangle's box; per axis with ext > 0 the bin clip(int((c - clo) (16f / ext)), 0, 15), every
              operation a singly rounded float32 one; the left set is exactly {bin <= b} for some axis and some b < 15 with both sides
              non-empty; with cost = half_area(L) |L| + half_area(R) |R| over the unpadded unions of the triangle boxes, in float64, the
              cost of the split taken is at most (1 + MARGIN) times the least over all such (axis, b)
MARGIN = 2e-6 is derived, not measured: a builder evaluates a cost in float32 through at most eight roundings of non-negative terms
in a row (two differences and their product: 3; the sum of three products: 5; times the count: 6; the sum of the two sides: 7), so its
relative error stays below 8 * 2^-24 < 5e-7; two costs are compared (1e-6) and the margin leaves a factor of two on top.  The bound
is relative, so it needs float32 half areas that are normal numbers: the verifier asserts a half area of at least 1e-30 for every node
it holds to the sah rule (with extents near 1e-29 every float32 cost is 0 and a builder rightly takes the first split).

Collapse checks on the same recovery: a four-wide node with fewer than four used children has only leaf children; the adoption order
(collapse_bvh4: largest surface first) is replayed on the recovered grouping, with the padded boxes of the adopted-away nodes recomputed
by bvh_tree_check.refit_pad and areas in float32 as ChildRef::area computes them: at each step the adopted child's area is at least
that of every other internal candidate (ties pass); nodes with an ambiguous grouping are skipped and counted.  check_wide: every used
child range of the sixteen-wide tree is one of the recovered binary node ranges.

Where the device builder is documented to differ (bf_build.hip, header: (1) WHICH triangles a forced cut puts left, (2) the order inside
a leaf and between equal-cost splits, (3) the node order) the rule above does not look: it speaks of counts, sets and costs only.

tests/test_sah_ref_host.py shows that the verifier accepts the host builder's trees and that it can fail."""
import numpy as np

from tests.bvh_tree_check import EMPTY, _children, _levels, refit_pad

f32, f64 = np.float32, np.float64
K_MAX_LEAF = 2
K_MAX_DEPTH = 31
K_BINS = 16
MARGIN = 2e-6
MIN_HALF_AREA = 1e-30


class SplitRuleError(AssertionError):
    pass


# ---- inputs the two test files share -----------------------------------------------------------------------------------------------
def clusters(sizes, seed=0):
    """(v, f): cluster i is sizes[i] triangles with centroids uniform in a unit cube at offset (4 i, 0.7 i, 0.3 i), vertices at
    centroid + 0.05 N(0, 1)"""
    rng = np.random.default_rng(seed)
    tri = []
    for i, m in enumerate(sizes):
        c = rng.uniform(0.0, 1.0, (m, 1, 3)) + np.array([4.0 * i, 0.7 * i, 0.3 * i])
        tri.append(c + 0.05 * rng.standard_normal((m, 3, 3)))
    v = np.concatenate(tri).reshape(-1, 3).astype(f32)
    return v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3)


def spiral(n=400, seed=0):
    """(v, f): triangle i sits at 0.92**i along a random unit direction and is 0.3 * 0.92**i large: SAH peels one triangle per level, so
    the depth budget runs out and the builders cut by count"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    s = 0.92 ** np.arange(n)
    v = (s[:, None, None] * (d[:, None, :] + 0.3 * rng.standard_normal((n, 3, 3)))).reshape(-1, 3).astype(f32)
    return v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def soup_with_copies(n=500, copies=40, seed=7):
    """(v, f): a triangle soup plus `copies` copies of one small triangle (their centroids coincide)"""
    from beifong_amd import meshgen
    v, _ = meshgen.triangle_soup(n, seed=seed)
    small = np.array([[0.31, -0.22, 0.13], [0.33, -0.21, 0.14], [0.32, -0.2, 0.11]], f32)
    v = np.concatenate([v, np.tile(small, (copies, 1))]).astype(f32)
    return v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3)


# ---- slot ranges -------------------------------------------------------------------------------------------------------------------
def slot_ranges(nodes, width):
    """(first, count) int64[n, W] of every child slot (count 0 for unused slots); asserts that every reference covers a contiguous slot
    range and that a node's children, taken in slot order, tile the node's range"""
    _, _, ref = _children(nodes, width)
    n, W = ref.shape
    first, count = np.zeros((n, W), np.int64), np.zeros((n, W), np.int64)
    if n == 0:
        return first, count
    shift, mask = (3, 7) if width == 4 else (4, 15)
    used = ref != EMPTY
    leaf = used & (ref < 0)
    enc = (~ref[leaf].astype(np.int64)) & 0xffffffff
    first[leaf], count[leaf] = enc >> shift, (enc & mask) + 1
    nfirst, ncount = np.zeros(n, np.int64), np.zeros(n, np.int64)
    big = np.int64(1) << 40
    for level in reversed(_levels(ref)):
        r = ref[level]
        internal = r >= 0
        c = r[internal].astype(np.int64)
        fl, cl = first[level], count[level]
        fl[internal], cl[internal] = nfirst[c], ncount[c]                 # (the level below is complete)
        first[level], count[level] = fl, cl
        u = used[level]
        key = np.where(u, fl, big)
        o = np.argsort(key, axis=1, kind="stable")
        sf, sc, su = np.take_along_axis(key, o, 1), np.take_along_axis(cl, o, 1), np.take_along_axis(u, o, 1)
        gap = su[:, 1:] & (sf[:, :-1] + sc[:, :-1] != sf[:, 1:])
        if gap.any():
            raise SplitRuleError(f"the children of {width}-wide node {int(level[np.argwhere(gap)[0, 0]])} do not tile a contiguous slot range")
        nfirst[level], ncount[level] = sf[:, 0], cl.sum(1)
    return first, count


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def _half_area64(lo, hi):
    d = hi.astype(f64) - lo.astype(f64)
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


def _area32(lo, hi):
    """ChildRef::area: d0 d1 + d1 d2 + d2 d0 in float32, left to right"""
    d = (np.asarray(hi, f32) - np.asarray(lo, f32)).astype(f32)
    return f32(f32(f32(d[0] * d[1]) + f32(d[1] * d[2])) + f32(d[2] * d[0]))


def _need(count):
    need = 0
    while (K_MAX_LEAF << need) < count:
        need += 1
    return need


class _Rule:
    def __init__(self, rows):
        xyz = np.ascontiguousarray(rows[:, :, :3], f32)
        self.lo, self.hi = xyz.min(1), xyz.max(1)
        self.cen = (f32(0.5) * (self.lo + self.hi)).astype(f32)
        self._cache = {}

    def box(self, first, count):
        return self.lo[first:first + count].min(0), self.hi[first:first + count].max(0)

    def prefetch(self, pairs):
        """the sweeps of many (first, count) at once, in classes of like size: the same arithmetic as one at a time"""
        todo = sorted({(int(f), int(c)) for f, c in pairs if c > K_MAX_LEAF and (int(f), int(c)) not in self._cache}, key=lambda fc: fc[1])
        at = 0
        while at < len(todo):
            P = max(8, 2 * todo[at][1])                              # the class: counts up to P, at most 2^16 padded slots a chunk
            end = at
            while end < len(todo) and todo[end][1] <= P and (end - at + 1) * P <= max(P, 1 << 16):
                end += 1
            P = todo[end - 1][1]
            self._sweep(np.array(todo[at:end], np.int64).reshape(-1, 2), P)
            at = end

    def _sweep(self, fc, P):
        first, count = fc[:, 0], fc[:, 1]
        live = np.arange(P)[None, :] < count[:, None]                                              # [m, P]
        idx = np.minimum(first[:, None] + np.arange(P)[None, :], len(self.lo) - 1)
        lo, hi, cen = self.lo[idx], self.hi[idx], self.cen[idx]                                    # [m, P, 3]
        inf = f32(np.inf)
        clo = np.where(live[..., None], cen, inf).min(1)
        ext = (np.where(live[..., None], cen, -inf).max(1) - clo).astype(f32)                      # [m, 3]
        axes = ext > 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            scale = np.where(axes, f32(K_BINS) / ext, f32(0)).astype(f32)
            t = ((cen - clo[:, None, :]).astype(f32) * scale[:, None, :]).astype(f32)
            bins = np.clip(np.where(axes[:, None, :] & live[..., None], t, f32(0)).astype(np.int32), 0, K_BINS - 1)      # (int) truncates; t >= 0
        oh = (bins[..., None] == np.arange(K_BINS, dtype=np.int32)) & live[:, :, None, None]       # [m, P, 3, 16]
        blo = np.where(oh[..., None], lo[:, :, None, None, :], inf).min(1)                         # [m, 3, 16, 3]
        bhi = np.where(oh[..., None], hi[:, :, None, None, :], -inf).max(1)
        cnt = oh.sum(1)                                                                            # [m, 3, 16]
        plo, phi = np.minimum.accumulate(blo, 2), np.maximum.accumulate(bhi, 2)
        slo, shi = np.minimum.accumulate(blo[:, :, ::-1], 2)[:, :, ::-1], np.maximum.accumulate(bhi[:, :, ::-1], 2)[:, :, ::-1]
        nl = cnt.cumsum(2)[:, :, :K_BINS - 1]
        nr = count[:, None, None] - nl
        valid = axes[:, :, None] & (nl > 0) & (nr > 0)
        with np.errstate(invalid="ignore"):
            cost = _half_area64(plo[:, :, :-1], phi[:, :, :-1]) * nl + _half_area64(slo[:, :, 1:], shi[:, :, 1:]) * nr
            cost = np.where(valid, cost, np.inf)                                                   # [m, 3, 15]
            ha = _half_area64(np.where(live[..., None], lo, inf).min(1), np.where(live[..., None], hi, -inf).max(1))
        least = cost.min((1, 2))
        for k in range(len(fc)):
            c = int(count[k])
            self._cache[(int(first[k]), c)] = (bins[k, :c], axes[k], cost[k], float(least[k]), float(ha[k])) if axes[k].any() else None

    def sweep(self, first, count):
        """None if the centroids coincide, else (bins int32[count, 3], axes bool[3], the 3 x 15 candidate costs (inf: no candidate), the
        least of them, the node's half area)"""
        key = (first, count)
        if key not in self._cache:
            self._sweep(np.array([key], np.int64), count)
        return self._cache[key]

    def allowed(self, first, count, depth, mid):
        """(kind, None) or (None, why not)"""
        if count <= K_MAX_LEAF:
            return None, f"({first}, {count}) is split, but at most {K_MAX_LEAF} triangles are a leaf"
        if depth + _need(count) + 1 >= K_MAX_DEPTH:
            return ("forced", None) if mid == count // 2 else (None, f"({first}, {count}) at depth {depth} must be cut at {count // 2}, not {mid}")
        sw = self.sweep(first, count)
        if sw is None:
            return ("coincident", None) if mid == count // 2 else (None, f"({first}, {count}): coincident centroids must be cut at {count // 2}, not {mid}")
        bins, axes, cost, least, ha = sw
        if not ha >= MIN_HALF_AREA:
            raise SplitRuleError(f"binary node ({first}, {count}): half area {ha!r} is below {MIN_HALF_AREA}: the relative margin means "
                                 "nothing where float32 half areas are not normal numbers")
        assert least < np.inf                        # (ext > 0 puts a triangle into bin 0 and another into bin 15)
        top, bottom = bins[:mid].max(0), bins[mid:].min(0)
        taken = [float(cost[a, top[a]]) for a in range(3) if axes[a] and top[a] < bottom[a]]          # the left set is {bin <= top[a]} of axis a
        if not taken:
            return None, f"({first}, {count}) cut at {mid}: the left set is no {{bin <= b}} of any axis"
        taken = min(taken)                           # (the same two sets whichever axis states them, hence the same cost)
        if taken <= (1.0 + MARGIN) * least:
            return "sah", None
        return None, f"({first}, {count}) cut at {mid}: cost {taken!r} against the least {least!r} (ratio - 1 = {taken / least - 1:.3e})"


def _groupings(i, j):
    """every binary tree over the ranges i .. j - 1 in order: an int (one range) or a pair (left, right)"""
    if j - i == 1:
        yield i
        return
    for m in range(i + 1, j):
        for left in _groupings(i, m):
            for right in _groupings(m, j):
                yield (left, right)


def _span(t):
    while isinstance(t, tuple):
        t = t[0]
    return t


def _end(t):
    while isinstance(t, tuple):
        t = t[1]
    return t + 1


class Recovered:
    """counts: {"sah", "forced", "coincident"}: binary nodes by the rule that allowed them, "ambiguous": four-wide nodes with more than
    one allowed grouping, "adoption_checked" / "adoption_skipped": four-wide nodes whose adoption order was replayed / skipped as
    ambiguous.  nodes: {(first, count, depth)} of the binary tree, leaves included, the union over every allowed grouping.
    prim_sets: the same nodes as sets of primitive words (the sorted words' bytes).  slot_sets: the sets under every child slot."""

    def __init__(self):
        self.counts = dict(sah=0, forced=0, coincident=0, ambiguous=0, adoption_checked=0, adoption_skipped=0)
        self.nodes, self.kinds = set(), {}
        self.prim_sets, self.slot_sets = set(), set()

    def ranges(self):
        return {(f, c) for f, c, _ in self.nodes}


def verify(nodes, rows, root, origin_scale):
    """Hold a four-wide tree to the split rule and the collapse rule; raises SplitRuleError, returns a Recovered.
    `origin_scale`: the ray-origin bound the boxes were padded for (capi.Scene.debug_origin_scale)."""
    out = Recovered()
    n_tris = rows.shape[0]
    prim = np.ascontiguousarray(rows).view(np.uint32)[:, 0, 3]

    def note(first, count, depth):
        out.nodes.add((first, count, depth))

    if n_tris == 0:
        return out
    if root < 0:
        if n_tris > K_MAX_LEAF:
            raise SplitRuleError(f"{n_tris} triangles in one leaf")
        note(0, n_tris, 0)
    else:
        rule = _Rule(rows)
        lo, hi, ref = _children(nodes, 4)
        first, count = slot_ranges(nodes, 4)
        used = ref != EMPTY
        if int(count[0].sum()) != n_tris or int(first[0][used[0]].min()) != 0:
            raise SplitRuleError("the root does not cover every slot")
        depths = {0: {0}}
        level = [0]
        while level:
            nxt, layout, pairs = [], {}, []
            for i in level:
                slots = sorted(np.flatnonzero(used[i]).tolist(), key=lambda k: first[i, k])
                starts = [int(first[i, k]) for k in slots] + [int(first[i, slots[-1]] + count[i, slots[-1]])]
                layout[i] = slots, starts
                pairs += [(starts[a], starts[b] - starts[a]) for a in range(len(slots)) for b in range(a + 2, len(slots) + 1)]
            rule.prefetch(pairs)
            for i in level:
                slots, starts = layout[i]
                k = len(slots)
                for s in slots:
                    if ref[i, s] >= 0 and count[i, s] <= K_MAX_LEAF:
                        raise SplitRuleError(f"node {i}: an internal child of {int(count[i, s])} triangles")
                    if ref[i, s] < 0 and count[i, s] > K_MAX_LEAF:
                        raise SplitRuleError(f"node {i}: a leaf of {int(count[i, s])} triangles")
                if k < 4 and any(ref[i, s] >= 0 for s in slots):
                    raise SplitRuleError(f"node {i} has {k} children, one of them internal: a node adopts until it has four children or only leaves")
                good, why = [], []
                for d0 in sorted(depths[i]):
                    for g in _groupings(0, k):
                        kinds, leaf_depth, ok = [], {}, True
                        stack = [(g, d0)]
                        while stack and ok:
                            t, d = stack.pop()
                            if not isinstance(t, tuple):
                                leaf_depth[t] = d
                                continue
                            a, m, b = starts[_span(t)], starts[_span(t[1])], starts[_end(t)]
                            kind, reason = rule.allowed(a, b - a, d, m - a)
                            if kind is None:
                                ok = False
                                why.append(reason)
                            kinds.append((a, b - a, d, kind))
                            stack += [(t[0], d + 1), (t[1], d + 1)]
                        if ok:
                            good.append((d0, g, kinds, leaf_depth))
                if not good:
                    raise SplitRuleError(f"four-wide node {i} (slot ranges {[(starts[j], starts[j + 1] - starts[j]) for j in range(k)]}, "
                                         f"depth {sorted(depths[i])}): no grouping of its children follows the split rule: " + "; ".join(dict.fromkeys(why)))
                if len(good) > 1:
                    out.counts["ambiguous"] += 1
                for d0, g, kinds, leaf_depth in good:
                    for a, c, d, kind in kinds:
                        note(a, c, d)
                        out.kinds[(a, c, d)] = kind
                    for j, d in leaf_depth.items():
                        s = slots[j]
                        note(starts[j], starts[j + 1] - starts[j], d)
                        if ref[i, s] >= 0:
                            depths.setdefault(int(ref[i, s]), set()).add(d)
                        elif d > K_MAX_DEPTH:
                            raise SplitRuleError(f"node {i}: a leaf at binary depth {d}")
                for j, s in enumerate(slots):
                    out.slot_sets.add(np.sort(prim[starts[j]:starts[j + 1]]).tobytes())
                    if ref[i, s] >= 0:
                        nxt.append(int(ref[i, s]))
                # the adoption order of collapse_bvh4, replayed
                if len(good) > 1:
                    out.counts["adoption_skipped"] += 1
                else:
                    out.counts["adoption_checked"] += 1
                    g = good[0][1]

                    def area(t):
                        if isinstance(t, tuple):
                            a, b = starts[_span(t)], starts[_end(t)]
                            plo, phi = refit_pad(*rule.box(a, b - a), origin_scale)
                            return _area32(plo, phi)
                        return _area32(lo[i, slots[t]], hi[i, slots[t]])

                    def internal(t):
                        return isinstance(t, tuple) or ref[i, slots[t]] >= 0

                    cur = [g[0], g[1]]
                    while any(isinstance(t, tuple) for t in cur):
                        cand = [(area(t), t) for t in cur if internal(t)]
                        a_best, t_best = max(((a, t) for a, t in cand if isinstance(t, tuple)), key=lambda x: x[0])
                        worst = max(a for a, _ in cand)
                        if not a_best >= worst:
                            raise SplitRuleError(f"four-wide node {i}: the collapse adopted a child of surface {a_best!r} while an internal "
                                                 f"candidate of surface {worst!r} stood beside it (largest surface first)")
                        cur[cur.index(t_best)] = t_best[0]
                        cur.append(t_best[1])
            level = nxt
    for kind in out.kinds.values():
        out.counts[kind] += 1
    for a, c, _ in out.nodes:
        out.prim_sets.add(np.sort(prim[a:a + c]).tobytes())
    return out


def check_wide(wnodes, wroot, n_tris, recovered):
    """Sixteen-wide tree: every used child range, leaves of up to 16 slots included, is one of the recovered binary node ranges.
    Returns the number of child ranges checked."""
    if n_tris == 0:
        return 0
    ranges = recovered.ranges()
    if wroot < 0:
        enc = ~int(wroot) & 0xffffffff
        if (enc >> 4, (enc & 15) + 1) != (0, n_tris):
            raise SplitRuleError("the sixteen-wide root leaf does not cover every slot")
        return 0
    first, count = slot_ranges(wnodes, 16)
    used = wnodes["c"]["child"] != EMPTY
    if int(count[0].sum()) != n_tris:
        raise SplitRuleError("the sixteen-wide root does not cover every slot")
    for f, c in zip(first[used].tolist(), count[used].tolist()):
        if (f, c) not in ranges:
            raise SplitRuleError(f"the sixteen-wide child range ({f}, {c}) is no node of the binary tree the four-wide tree came from")
    return int(used.sum())
