"""The sequential statement of the steering shortcut (include/mpfmt.h, "steering shortcut") in plain Python: working path with leg costs,
the cum fold, ok(i, j), shortcut (src/postprocessors.jl:6-16 with ok in the place of is_free_motion), refine and the driver -- the
normative procedure the device batch (mpfmt_steer_shortcut_batch) is compared with, bit for bit.  Python floats are IEEE binary64 and
CPython never fuses a * b + c.

The space enters through two callables only:
    pair(v, w) -> (cost, dur, bit, nseg)       the steer's cost and duration, the motion test's bit and its segment count
    mid(v, w)  -> state                         the state at fl(T / 2) of the steered trajectory v -> w
so the same code runs over the device's own primitive (exactness of the procedure) and over the CPU oracle (independence).
Shared by tests/test_steershortcut_cpu.py and tests/test_gpu_steershortcut.py (a helper module, not a test file)."""
import numpy as np

SLACK = 1.0 + 2.0 ** -30
DONE, TRUNCATED = 0, 1


class Asker:
    """pair(v, w) with the counts of the sequential procedure: `asked` tests, `checks` = the sum of their nseg.  Results are remembered
    by the bytes of the pair (the procedure asks some pairs again in later passes; the counts still grow).  `margins` collects
    |lhs - threshold| / threshold of every acceptance comparison."""

    def __init__(self, pair):
        self.pair, self.memo = pair, {}
        self.asked = self.checks = 0
        self.margins = []

    def __call__(self, v, w):
        key = (v.tobytes(), w.tobytes())
        if key not in self.memo:
            c, t, b, n = self.pair(v, w)
            self.memo[key] = (float(c), float(t), bool(b), int(n))
        r = self.memo[key]
        self.asked += 1
        self.checks += r[3]
        return r

    def compare(self, lhs, thr):
        """lhs <= thr, remembering how close it was"""
        if thr > 0 and np.isfinite(lhs):
            self.margins.append(abs(lhs - thr) / thr)
        return lhs <= thr


class Path:
    """states p[i], the cost c[i] and the duration t[i] of the leg that leaves state i (n - 1 of each), origin org[i]"""

    def __init__(self, p, c, t, org):
        self.p, self.c, self.t, self.org = p, c, t, org

    def __len__(self):
        return len(self.p)

    def same_states(self, other):
        return len(self) == len(other) and all(a.tobytes() == b.tobytes() for a, b in zip(self.p, other.p))


def fold(c):
    cum = [0.0]
    for x in c:
        cum.append(cum[-1] + x)
    return cum


def split_index(lo, hi):
    """the state a blocked node (lo, hi) is split at: mid = ceil(N / 2) of its N = hi - lo + 1 states (postprocessors.jl:13)"""
    return lo + -(-(hi - lo + 1) // 2) - 1


def shortcut(W, ask, stats):
    """One shortcut(path): -> the new Path.  stats["nodes"] gains the inner nodes of the split tree of len(W) (what a speculating device
    evaluates), stats["accepted"] the replacements made."""
    n = len(W)
    cum = fold(W.c)
    if n > 2:
        stats["nodes"] += n - 2

    def rec(lo, hi):                                          # the legs of the result between states lo and hi: [(state, cost, dur)]
        if hi - lo == 1:
            return [(lo, W.c[lo], W.t[lo])]
        cost, dur, bit, _ = ask(W.p[lo], W.p[hi])
        span = cum[hi] - cum[lo]
        thr = SLACK * span
        near = ask.compare(cost, thr)
        if bit and near:
            stats["accepted"] += 1
            return [(lo, cost, dur)]
        s = split_index(lo, hi)
        return rec(lo, s) + rec(s, hi)

    legs = rec(0, n - 1)
    keep = [i for i, _, _ in legs] + [n - 1]
    return Path([W.p[i] for i in keep], [c for _, c, _ in legs], [t for _, _, t in legs], [W.org[i] for i in keep])


def fixed_point(W, ask, stats):
    while True:
        if len(W) <= 2:
            return W
        S = shortcut(W, ask, stats)
        if len(S) == len(W):                                  # shortcut only removes states: equal length = equal path
            return S
        W = S


def refine(W, ask, mid, stats):
    """-> (the expanded Path, states inserted)"""
    p, c, t, org = [], [], [], []
    k = 0
    for i in range(len(W) - 1):
        ins = False
        if W.t[i] > 0:
            m = np.ascontiguousarray(mid(W.p[i], W.p[i + 1]), dtype=np.float64)
            c1, t1, b1, _ = ask(W.p[i], m)
            c2, t2, b2, _ = ask(m, W.p[i + 1])
            stats["proposed"] += 1
            s = c1 + c2
            thr = SLACK * W.c[i]
            near = ask.compare(s, thr)
            ins = b1 and b2 and near
        if ins:
            p += [W.p[i], m]; c += [c1, c2]; t += [t1, t2]; org += [W.org[i], 0]
            k += 1
            stats["accepted"] += 1
        else:
            p.append(W.p[i]); c.append(W.c[i]); t.append(W.t[i]); org.append(W.org[i])
    p.append(W.p[-1]); org.append(W.org[-1])
    return Path(p, c, t, org), k


def steer_shortcut(path, pair, mid, iterations=4, max_states=256):
    """-> (states (n_out, d), cumcost, origin, info, asker).  info carries every field of mpfmt_steer_shortcut_info; tests_evaluated is
    what a device that tests the whole split tree of every pass runs: the input legs, n - 2 nodes per pass, two halves per proposing
    leg.  info["accepted"] (not a field of the struct) counts the replacements made, for the cost property."""
    P = [np.ascontiguousarray(x, dtype=np.float64) for x in path]
    ask = Asker(pair)
    stats = {"nodes": 0, "proposed": 0, "accepted": 0}
    n0 = len(P)
    c, t, blocked = [], [], 0
    for i in range(n0 - 1):
        ci, ti, bi, _ = ask(P[i], P[i + 1])
        c.append(ci); t.append(ti)
        blocked += 0 if bi else 1
    cost_in = fold(c)[-1]
    W = fixed_point(Path(P, c, t, list(range(1, n0 + 1))), ask, stats)
    status, done, maxlen, inserted = DONE, 0, n0, 0
    for _ in range(iterations):
        N, k = refine(W, ask, mid, stats)
        if len(N) > max_states:
            status = TRUNCATED
            break
        begin = W
        inserted += k
        maxlen = max(maxlen, len(N))
        W = fixed_point(N, ask, stats)
        done += 1
        if W.same_states(begin):
            break
    cum = fold(W.c)
    info = dict(status=status, iterations_done=done, n_out=len(W), max_working_len=maxlen, inserted=inserted, legs_blocked=blocked,
                collision_checks=ask.checks, tests_evaluated=(n0 - 1) + stats["nodes"] + 2 * stats["proposed"], cost_in=cost_in,
                cost_out=cum[-1], accepted=stats["accepted"])
    return np.array(W.p), np.array(cum), np.array(W.org, dtype=np.int32), info, ask


# ---- the Euclidean split tree, for the comparison of test_steershortcut_cpu.py ------------------------------------------------------
def table_pair(bits):
    """pair() over integer "states" (1-vectors holding an index) whose bit comes from a table {(i, j): bool}; unit leg costs make the
    cost condition hold for every pair (cost 0 <= any span), so ok is the plain bit table."""
    def pair(v, w):
        i, j = int(v[0]), int(w[0])
        return (1.0 if j == i + 1 else 0.0), 1.0, bits(i, j), 1
    return pair
