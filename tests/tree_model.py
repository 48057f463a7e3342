"""numpy restatement of the Barnes-Hut force (NB_FORCE_TREE, include/nbody.h) used by the tree tests.

Everything is float32 with one rounding per operation.  Two builders give the same tree:

``build_serial``      inserts the bodies one by one in index order, one body per leaf, splitting a leaf into four children in
                      quadrant order until two positions part; centres of mass afterwards, parents in reverse creation order.
                      Node indices follow the insertion order.
``build_canonical``   the construction the GPU uses: every body's quadrant path from the root (found by descending with the
                      rounded child centres), bodies sorted by (path, index), nodes laid out in pre-order.  Node indices do
                      not depend on the body order.

``walk`` evaluates the accelerations of all bodies on either layout and can return, per body, the nodes it accepted.
A tree is a dict of arrays: px, py, mass, s2 (cell size squared), child (first child, 0 = leaf), next (-1 = end), depth.
"""
from __future__ import annotations

import numpy as np

F = np.float32
DEPTH_CAP = 63          # levels a path is followed for: nb_tree.hip.h TREE_DEPTH_CAP
HALF = F(0.5)


def root_cell(x, y):
    """Centre and size of the cell containing all bodies: ((min + max) * 0.5, max extent)."""
    lo_x, hi_x, lo_y, hi_y = x.min(), x.max(), y.min(), y.max()
    cx, cy = (lo_x + hi_x) * HALF, (lo_y + hi_y) * HALF
    ex, ey = hi_x - lo_x, hi_y - lo_y
    return F(cx), F(cy), F(max(ex, ey))


def quadrant(px, py, cx, cy):
    return ((py > cy).astype(np.int64) << 1) | (px > cx).astype(np.int64)


def child_cell(cx, cy, size, q):
    """Child q of cell (cx, cy, size): half the size, centre moved by (+-0.5) * new size per axis."""
    ns = F(size * HALF)
    ox = F(F(q & 1) - HALF)
    oy = F(F(q >> 1) - HALF)
    return F(cx + F(ox * ns)), F(cy + F(oy * ns)), ns


# ---------------------------------------------------------------------------------------------------------------------
# serial insertion
# ---------------------------------------------------------------------------------------------------------------------
def build_serial(x, y, m) -> dict:
    x, y, m = (np.ascontiguousarray(a, F) for a in (x, y, m))
    rcx, rcy, rsize = root_cell(x, y)
    px, py, mass, cx, cy, size, child, nxt, depth = [F(0)], [F(0)], [F(0)], [rcx], [rcy], [rsize], [0], [-1], [0]
    parents = []
    for b in range(x.shape[0]):
        bx, by, bm = x[b], y[b], m[b]
        if bm == 0:                                        # a massless body is not inserted (a tracer)
            continue
        node = 0
        while child[node]:
            node = child[node] + int(((by > cy[node]) << 1) | (bx > cx[node]))
        if mass[node] == 0:
            px[node], py[node], mass[node] = bx, by, bm
            continue
        ex, ey, em = px[node], py[node], mass[node]
        if bx == ex and by == ey:
            mass[node] = F(mass[node] + bm)
            continue
        while True:
            first = len(px)
            child[node] = first
            parents.append(node)
            for q in range(4):
                ccx, ccy, cs = child_cell(cx[node], cy[node], size[node], q)
                px.append(F(0)); py.append(F(0)); mass.append(F(0)); cx.append(ccx); cy.append(ccy); size.append(cs)
                child.append(0); nxt.append(first + q + 1 if q < 3 else nxt[node]); depth.append(depth[node] + 1)
            q1 = int(((ey > cy[node]) << 1) | (ex > cx[node]))
            q2 = int(((by > cy[node]) << 1) | (bx > cx[node]))
            if depth[node] + 1 > DEPTH_CAP:
                raise OverflowError("two positions are not separated within the depth cap")
            if q1 == q2:
                node = first + q1
                continue
            px[first + q1], py[first + q1], mass[first + q1] = ex, ey, em
            px[first + q2], py[first + q2], mass[first + q2] = bx, by, bm
            break
    for node in reversed(parents):
        sx, sy, sm = F(0), F(0), F(0)
        for q in range(4):
            c = child[node] + q
            sx = F(sx + F(px[c] * mass[c])); sy = F(sy + F(py[c] * mass[c])); sm = F(sm + mass[c])
        if sm > 0:
            inv = F(F(1) / sm)
            sx, sy = F(sx * inv), F(sy * inv)
        px[node], py[node], mass[node] = sx, sy, sm
    size = np.array(size, F)
    return {"px": np.array(px, F), "py": np.array(py, F), "mass": np.array(mass, F), "s2": size * size,
            "child": np.array(child, np.int64), "next": np.array(nxt, np.int64), "depth": np.array(depth, np.int64)}


# ---------------------------------------------------------------------------------------------------------------------
# canonical construction
# ---------------------------------------------------------------------------------------------------------------------
def path_digits(x, y, root, levels: int = DEPTH_CAP) -> np.ndarray:
    """(n, levels) uint8: the quadrant taken at every level when descending from the root with the rounded child centres."""
    cx = np.full(x.shape, root[0], F)
    cy = np.full(x.shape, root[1], F)
    size = root[2]
    out = np.zeros((x.shape[0], levels), np.uint8)
    for l in range(levels):
        q = quadrant(x, y, cx, cy)
        out[:, l] = q
        size = F(size * HALF)
        cx = cx + ((q & 1).astype(F) - HALF) * size
        cy = cy + ((q >> 1).astype(F) - HALF) * size
    return out


def build_canonical(x, y, m) -> dict:
    x, y, m = (np.ascontiguousarray(a, F) for a in (x, y, m))
    root = root_cell(x, y)
    ins = np.nonzero(m != 0)[0]
    dig = path_digits(x[ins], y[ins], root)
    order = np.lexsort((ins,) + tuple(dig[:, l] for l in range(DEPTH_CAP - 1, -1, -1)))
    ins, dig = ins[order], dig[order]
    k = ins.shape[0]
    head = np.ones(k, bool)
    if k > 1:
        head[1:] = (dig[1:] != dig[:-1]).any(axis=1)
        same = ~head[1:]
        if ((x[ins[1:]] != x[ins[:-1]]) | (y[ins[1:]] != y[ins[:-1]]))[same].any():
            raise OverflowError("two positions are not separated within the depth cap")
    first = np.nonzero(head)[0]
    last = np.append(first[1:], k)
    U = first.shape[0]
    udig = dig[first]
    upx, upy = x[ins[first]], y[ins[first]]
    um = np.zeros(U, F)
    for u in range(U):                                   # coincident bodies: masses added in ascending body index
        s = m[ins[first[u]]]
        for j in range(first[u] + 1, last[u]):
            s = F(s + m[ins[j]])
        um[u] = s
    size_of = [root[2]]
    for _ in range(DEPTH_CAP + 1):
        size_of.append(F(size_of[-1] * HALF))
    px, py, mass, s2, child, nxt, depth = [], [], [], [], [], [], []

    def emit(d, bx=F(0), by=F(0), bm=F(0), branch=False):
        px.append(bx); py.append(by); mass.append(bm); s2.append(F(size_of[d] * size_of[d]))
        child.append(len(px) if branch else 0); nxt.append(-1); depth.append(d)
        return len(px) - 1

    # pre-order, iteratively: the stack holds (range of points, depth) still to emit, and closing markers that set `next`
    stack = [(0, U, 0)]
    while stack:
        item = stack.pop()
        if len(item) == 1:
            nxt[item[0]] = len(px)
            continue
        a, b, d = item
        if b - a == 0:
            node = emit(d)
            nxt[node] = len(px)
        elif b - a == 1:
            node = emit(d, upx[a], upy[a], um[a])
            nxt[node] = len(px)
        else:
            node = emit(d, branch=True)
            cuts = a + np.searchsorted(udig[a:b, d], [0, 1, 2, 3, 4])
            stack.append((node,))
            for q in (3, 2, 1, 0):
                stack.append((int(cuts[q]), int(cuts[q + 1]), d + 1))
    total = len(px)
    nxt = [(-1 if v == total else v) for v in nxt]
    for node in range(total - 1, -1, -1):
        if not child[node]:
            continue
        sx, sy, sm = F(0), F(0), F(0)
        c = child[node]
        for _ in range(4):
            sx = F(sx + F(px[c] * mass[c])); sy = F(sy + F(py[c] * mass[c])); sm = F(sm + mass[c])
            c = nxt[c] if nxt[c] >= 0 else total
        if sm > 0:
            inv = F(F(1) / sm)
            sx, sy = F(sx * inv), F(sy * inv)
        px[node], py[node], mass[node] = sx, sy, sm
    return {"px": np.array(px, F), "py": np.array(py, F), "mass": np.array(mass, F), "s2": np.array(s2, F),
            "child": np.array(child, np.int64), "next": np.array(nxt, np.int64), "depth": np.array(depth, np.int64)}


# ---------------------------------------------------------------------------------------------------------------------
# walk
# ---------------------------------------------------------------------------------------------------------------------
def quake_rsqrt(v):
    v = np.ascontiguousarray(v, F)
    yq = (np.uint32(0x5F3759DF) - (v.view(np.uint32) >> np.uint32(1))).view(F)
    return yq * (F(1.5) - (v * HALF * yq * yq))


def walk(tree: dict, x, y, eps: float, theta: float = 1.0, quake: bool = True, visited: bool = False):
    """Accelerations (ax, ay) of every body, all bodies advancing through the tree together; with ``visited`` also the
    (body, node) pairs that were accepted, in visit order per body."""
    x, y = np.ascontiguousarray(x, F), np.ascontiguousarray(y, F)
    n = x.shape[0]
    e2 = F(F(eps) * F(eps))
    t2 = F(F(theta) * F(theta))
    ax, ay = np.zeros(n, F), np.zeros(n, F)
    node = np.zeros(n, np.int64)
    live = np.arange(n)
    acc_pairs = []
    with np.errstate(all="ignore"):
        while live.size:
            nd = node[live]
            dx, dy = tree["px"][nd] - x[live], tree["py"][nd] - y[live]
            d2 = dx * dx + dy * dy
            far = tree["s2"][nd] < d2 * t2
            add = far & (d2 > 0)
            if add.any():
                t = d2[add] + e2
                inv = quake_rsqrt(t) if quake else (F(1) / np.sqrt(t)).astype(F)
                inv3 = inv * inv * inv
                s = tree["mass"][nd[add]] * inv3
                who = live[add]
                ax[who] = ax[who] + dx[add] * s
                ay[who] = ay[who] + dy[add] * s
                if visited:
                    acc_pairs.append(np.stack([who, nd[add]], axis=1))
            descend = ~far & (tree["child"][nd] != 0)
            new = np.where(descend, tree["child"][nd], tree["next"][nd])
            node[live] = new
            live = live[new >= 0]
    if visited:
        pairs = np.concatenate(acc_pairs) if acc_pairs else np.zeros((0, 2), np.int64)
        return ax, ay, pairs
    return ax, ay


def resum_f64(tree: dict, x, y, pairs: np.ndarray, eps: float):
    """The accepted (body, node) pairs summed in float64 with an exact 1/sqrt."""
    n = x.shape[0]
    b, nd = pairs[:, 0], pairs[:, 1]
    dx = tree["px"][nd].astype(np.float64) - x[b].astype(np.float64)
    dy = tree["py"][nd].astype(np.float64) - y[b].astype(np.float64)
    r2 = dx * dx + dy * dy + float(eps) ** 2
    s = tree["mass"][nd].astype(np.float64) / (r2 * np.sqrt(r2))
    return np.bincount(b, dx * s, n), np.bincount(b, dy * s, n)


def accelerations(x, y, m, eps, theta=1.0, quake=True, canonical=True):
    tree = (build_canonical if canonical else build_serial)(x, y, m)
    return walk(tree, x, y, eps, theta, quake)


def step(st: dict, eps: float, dt: float, nsteps: int = 1, theta: float = 1.0, clamp: bool = False, canonical: bool = True) -> dict:
    """Kick-drift steps in place on a float32 state (x, y, vx, vy, ax, ay, m), every operation rounded on its own; ``clamp``
    applies |v| <= 1000 after the kick.  The soft boundary is not restated here: no body may be beyond 80 000."""
    h = F(dt)
    for _ in range(nsteps):
        assert (st["x"] * st["x"] + st["y"] * st["y"] <= F(80000.0) * F(80000.0)).all()
        st["ax"], st["ay"] = accelerations(st["x"], st["y"], st["m"], eps, theta, True, canonical)
        st["vx"] = st["vx"] + st["ax"] * h
        st["vy"] = st["vy"] + st["ay"] * h
        if clamp:
            vm = st["vx"] * st["vx"] + st["vy"] * st["vy"]
            over = vm > F(1000.0) * F(1000.0)
            scale = np.where(over, F(1000.0) / np.sqrt(np.where(over, vm, F(1))), F(1)).astype(F)
            st["vx"] = np.where(over, st["vx"] * scale, st["vx"])
            st["vy"] = np.where(over, st["vy"] * scale, st["vy"])
        st["x"] = st["x"] + st["vx"] * h
        st["y"] = st["y"] + st["vy"] * h
    return st


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
