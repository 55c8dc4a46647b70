"""Pure-Python restatement of shortcut / cut_corner / adaptive_shortcut (src/postprocessors.jl:6-39) over a free(v, w) predicate, with the
two guards include/mpfmt.h documents ("adaptive shortcutting": max_states, stuck corners) -- the normative statement the host reference
(mpfmt_host_adaptive_shortcut) and the device batch (mpfmt_adaptive_shortcut_batch) are compared with, bit for bit.  Python floats are
IEEE binary64 and CPython never fuses a * b + c.  Shared by tests/test_shortcut_cpu.py and tests/test_gpu_shortcut.py (a helper module,
not a test file)."""
import math
import random

import jl_transliteration as jl

DONE, TRUNCATED, STUCK = 0, 1, 2


class Stuck(Exception):
    pass


class Counter:
    """free(v, w) of a world plus the two counts: `asked` = every test, `count` = the checker's own counter (boxesND.jl:26 -- reached
    only when the first point lies inside the state bounds, statespaces.jl:155)."""

    def __init__(self, free_counting):
        self.free_counting = free_counting          # (v, w, CC) -> bool, increments CC["count"] as the reference does
        self.CC = {"count": 0}
        self.asked = 0

    def __call__(self, v, w):
        self.asked += 1
        return self.free_counting(v, w, self.CC)


def boxes_counter(boxes, ss_lo, ss_hi):
    def f(v, w, CC):
        CC["boxes"] = boxes
        return jl.is_free_motion(v, w, boxes, ss_lo, ss_hi, CC)
    return Counter(f)


def sat2d_counter(obstacles, ss_lo, ss_hi):
    def f(v, w, CC):
        if ss_lo is not None and not jl.in_state_space(v, ss_lo, ss_hi):
            return False
        CC["count"] += 1
        return jl.is_free_motion_2d(v, w, obstacles)
    return Counter(f)


def shortcut(path, free):                                   # postprocessors.jl:6-16
    N = len(path)
    if N == 2:
        return path
    if free(path[0], path[-1]):
        return [path[0], path[-1]]
    mid = -(-N // 2)                                        # ceil(Int, N/2)
    return shortcut(path[:mid], free)[:-1] + shortcut(path[mid - 1:], free)


def cut_corner(v1, v2, v3, free, stats):                    # postprocessors.jl:18-26
    m1 = [(a + b) / 2 for a, b in zip(v1, v2)]
    m2 = [(a + b) / 2 for a, b in zip(v3, v2)]
    halvings = 0
    try:
        while not free(m1, m2):
            n1 = [(a + b) / 2 for a, b in zip(m1, v2)]
            n2 = [(a + b) / 2 for a, b in zip(m2, v2)]
            halvings += 1
            if n1 == m1 and n2 == m2:                       # guard 2: the reference would loop forever
                raise Stuck()
            m1, m2 = n1, n2
    finally:
        stats["max_halvings"] = max(stats["max_halvings"], halvings)
    return [v1, m1, m2, v3]


def fixed_point(path, free):
    while True:
        short = shortcut(path, free)
        if len(short) == len(path):                         # shortcut only removes states: equal length = equal path
            return short
        path = short


def adaptive_shortcut(path, free, iterations=10, max_states=256):      # postprocessors.jl:28-39
    """Returns (path, cumcost, info); free is a Counter."""
    path = [list(map(float, p)) for p in path]
    stats = {"max_halvings": 0}
    status, done, maxlen = DONE, 0, len(path)
    path = fixed_point(path, free)
    for _ in range(iterations):
        if 2 * len(path) - 2 > max_states:                  # guard 1
            status = TRUNCATED
            break
        try:
            new = path[0:1]
            for j in range(1, len(path) - 1):
                new += cut_corner(path[j - 1], path[j], path[j + 1], free, stats)[1:3]
            new += path[-1:]
        except Stuck:
            status = STUCK
            break
        path = new
        maxlen = max(maxlen, len(path))
        path = fixed_point(path, free)
        done += 1
    cum = [0.0]
    for a, b in zip(path[:-1], path[1:]):
        cum.append(cum[-1] + math.sqrt(jl.sqeuclid(b, a)))
    info = dict(status=status, iterations_done=done, n_out=len(path), max_working_len=maxlen, max_halvings=stats["max_halvings"],
                collision_checks=free.CC["count"], tests_asked=free.asked)
    return path, cum, info


def box_world(d, N, nb, seed):
    """The random box worlds of the shortcut tests: Random(seed) draws, in order, nb boxes (centre in [.2, .8]^d, then half-widths in
    [.05, .2]^d) and then the N - 1 uniform samples that follow init = (.05, ...).  Returns (boxes [(lo, hi)], V)."""
    rng = random.Random(seed)
    boxes = []
    for _ in range(nb):
        c = [rng.uniform(.2, .8) for _ in range(d)]
        h = [rng.uniform(.05, .2) for _ in range(d)]
        boxes.append(([c[i] - h[i] for i in range(d)], [c[i] + h[i] for i in range(d)]))
    V = [[.05] * d] + [[rng.random() for _ in range(d)] for _ in range(N - 1)]
    return boxes, V
