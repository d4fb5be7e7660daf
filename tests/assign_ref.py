"""The assignment procedure of include/codetr_assign.h restated in numpy with int64: shortest augmenting paths over the
costs -g, rows inserted in ascending order, the next column the unvisited one of the least distance with ties to the
lowest index, one dual update per augmentation.  `solve(G)` -> (match [n] int64 with -1 for unmatched, total, rounds);
`rounds` counts the relax-and-pick rounds, the unit the kernel's cost is measured in.  The tests compare the kernel's
matches with this element for element and both totals with scipy's optimum."""
import numpy as np

MAX_GAIN = (1 << 21) + 1
INF = np.int64(1) << np.int64(62)


def solve(G):
    G = np.clip(np.asarray(G, np.int64), 0, MAX_GAIN)
    n, m = G.shape
    M = max(n, m)
    C = np.zeros((n, M), np.int64)
    C[:, :m] = -G                                   # virtual columns: gain 0
    u, v = np.zeros(n, np.int64), np.zeros(M, np.int64)
    owner = np.full(M, -1, np.int64)
    pred = np.full(M, -1, np.int64)
    rounds = 0
    for i in range(n):
        dist = np.full(M, INF, np.int64)
        visited = np.zeros(M, bool)
        r, through, D, sink = i, -1, np.int64(0), -1
        for _ in range(M + 1):
            rounds += 1
            d = D + C[r] - u[r] - v
            better = ~visited & (d < dist)
            dist[better] = d[better]
            pred[better] = through
            j = int(np.argmin(np.where(visited, INF, dist)))   # the first of the minima: the lowest column
            D = dist[j]
            visited[j] = True
            if owner[j] < 0:
                sink = j
                break
            r, through = int(owner[j]), j
        assert sink >= 0, "a free column always exists"
        delta = D - dist[visited]
        v[visited] -= delta
        owned = owner[visited] >= 0
        u[owner[visited][owned]] += delta[owned]
        u[i] += D
        j = sink
        while j >= 0:
            p = int(pred[j])
            owner[j] = i if p < 0 else owner[p]
            j = p
    match = np.full(n, -1, np.int64)
    total = 0
    for j in range(m):
        r = int(owner[j])
        if r >= 0 and G[r, j] > 0:
            match[r] = j
            total += int(G[r, j])
    return match, total, rounds


def check_matching(G, match):
    """`match` is a matching of G's rows to its columns and every matched pair has a positive gain -> its total"""
    G = np.clip(np.asarray(G, np.int64), 0, MAX_GAIN)
    match = np.asarray(match)
    assert match.shape == (G.shape[0],)
    rows = np.flatnonzero(match >= 0)
    cols = match[rows]
    assert (match >= -1).all() and (cols < G.shape[1]).all() and len(set(cols.tolist())) == len(cols)
    assert (G[rows, cols] > 0).all()
    return int(G[rows, cols].sum())


def optimum(G):
    """scipy's optimum of the same (clamped) gains"""
    from scipy.optimize import linear_sum_assignment

    G = np.clip(np.asarray(G, np.int64), 0, MAX_GAIN)
    r, c = linear_sum_assignment(G, maximize=True)
    return int(G[r, c].sum())
