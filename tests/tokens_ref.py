"""Test oracle for sequences of int items (test-only): the scalar path of src/levenshtein.rs:471-532 restated over any items that
compare with ==, with the traceback of :561-606 and its tie order (substitution, then a_gap on <, then b_gap on <; transposition wins
ties with <=), the shorter sequence on the rows (:386-390).  The C oracle takes bytes only; this one is pinned against it on pairs
that map to bytes (test_tokens_cpu.py)."""

INF = float("inf")
_NAMES = ("Match", "Mismatch", "AGap", "BGap", "Transpose")


def _costs(c):
    if hasattr(c, "mismatch_cost"):
        return c.mismatch_cost, c.gap_cost, c.start_gap_cost, c.transpose_cost
    return tuple(c)


def levenshtein(a, b, k=None, trace_on=False, costs=(1, 1, 0, None)):
    """-> None (distance above k) | (distance, None | [(name, count), ...])"""
    mc, gc, sg, tc = _costs(costs)
    a, b = list(a), list(b)
    swap = len(a) > len(b)
    x, y = (b, a) if swap else (a, b)
    n, m = len(x), len(y)
    if n == 0 and m == 0:
        return (0, [] if trace_on else None) if (k is None or k >= 0) else None
    sgc = sg + gc
    col0 = lambda i: i * gc + sg if i else 0
    dp = [[0] * (m + 1) for _ in range(n + 1)]
    A = [[INF] * (m + 1) for _ in range(n + 1)]
    B = [[INF] * (m + 1) for _ in range(n + 1)]
    code = [[0] * (m + 1) for _ in range(n + 1)]
    for j in range(m + 1):
        dp[0][j] = col0(j)
    for i in range(1, n + 1):
        dp[i][0] = col0(i)
        xi, row, prev = x[i - 1], dp[i], dp[i - 1]
        for j in range(1, m + 1):
            A[i][j] = min(row[j - 1] + sgc, A[i][j - 1] + gc)
            B[i][j] = min(prev[j] + sgc, B[i - 1][j] + gc)
            sub = prev[j - 1] + (0 if xi == y[j - 1] else mc)
            ga, gb = A[i][j], B[i][j]
            v = min(sub, ga, gb)
            c = 2 if gb < min(sub, ga) else (1 if ga < sub else 0)
            if tc is not None and i >= 2 and j >= 2 and xi == y[j - 2] and x[i - 2] == y[j - 1]:
                tv = dp[i - 2][j - 2] + tc
                if tv <= v:
                    c = 3
                v = min(v, tv)
            row[j] = v
            code[i][j] = c
    d = dp[n][m]
    if k is not None and d > k:
        return None
    if not trace_on:
        return (d, None)
    runs = []
    i, j = n, m
    while i > 0 or j > 0:
        c = 1 if i == 0 else (2 if j == 0 else code[i][j])
        if c == 0:
            i -= 1; j -= 1
            e = 0 if x[i] == y[j] else 1
        elif c == 1:
            j -= 1
            e = 3 if swap else 2
        elif c == 2:
            i -= 1
            e = 2 if swap else 3
        else:
            i -= 2; j -= 2
            e = 4
        if runs and runs[-1][0] == e:
            runs[-1][1] += 1
        else:
            runs.append([e, 1])
    return (d, [(_NAMES[e], c) for e, c in reversed(runs)])


def codes(a, b):
    """an equality-preserving byte coding of one pair (any one: the distances and scripts do not depend on it), or None when the
    pair has more than 256 distinct items in all"""
    vals = {}
    for v in list(a) + list(b):
        vals.setdefault(v, len(vals))
    if len(vals) > 256:
        return None
    return bytes(vals[v] for v in a), bytes(vals[v] for v in b)
