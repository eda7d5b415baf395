"""Oracle for csrc/linkage.hip: the nearest-neighbour chain and the host labelling restated in numpy fp64, operation for
operation (feature sums in index order, the Lance-Williams rules on distances with the kernel's operand order), and
independent of the kernel.  tests/test_linkage.py pins it to scipy.cluster.hierarchy.linkage; the GPU tests compare
the device with it, so they need no scipy."""
import numpy as np

LINKAGES = ("ward", "complete", "single", "average")
METRICS = ("euclidean", "manhattan", "cosine")


def pairwise(X, metric="euclidean"):
    """[n, n] fp64 distances of the fp32 rows of X, +inf on the diagonal; every sum runs over the features in order."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    n, d = X.shape
    acc = np.zeros((n, n))
    if metric == "cosine":
        sq = np.zeros(n)
    for k in range(d):
        col = X[:, k]
        if metric == "euclidean":
            t = col[:, None] - col[None, :]
            acc += t * t
        elif metric == "manhattan":
            acc += np.abs(col[:, None] - col[None, :])
        elif metric == "cosine":
            acc += col[:, None] * col[None, :]
            sq += col * col
        else:
            raise ValueError(metric)
    if metric == "euclidean":
        D = np.sqrt(acc)
    elif metric == "manhattan":
        D = acc
    else:
        norm = np.sqrt(sq)
        cs = acc / (norm[:, None] * norm[None, :])
        cs = np.where(np.abs(cs) > 1.0, np.copysign(1.0, cs), cs)
        D = 1.0 - cs
    np.fill_diagonal(D, np.inf)
    return D


def _lance_williams(method, dak, dbk, dab, na, nb, nk):
    if method == "ward":
        return np.sqrt((((na + nk) * (dak * dak) + (nb + nk) * (dbk * dbk)) - nk * (dab * dab)) / ((na + nb) + nk))
    if method == "complete":
        return np.maximum(dak, dbk)
    if method == "single":
        return np.minimum(dak, dbk)
    if method == "average":
        return (na * dak + nb * dbk) / (na + nb)
    raise ValueError(method)


def nn_chain(D, method):
    """Raw merges in the order the chain finds them: (retired index, kept index) int64 [n-1, 2], heights, sizes.
    D is consumed."""
    n = D.shape[0]
    size = np.ones(n, dtype=np.int64)
    index = np.arange(n)
    chain = []
    merges, heights, sizes = [], [], []
    lowest = 0
    while len(merges) < n - 1:
        if not chain:
            while size[lowest] == 0:
                lowest += 1
            chain.append(lowest)
        x = chain[-1]
        cand = np.where((size > 0) & (index != x), D[x], np.inf)
        y = int(np.argmin(cand))                     # the smallest value, the lowest index among equals
        if not (size[y] > 0 and y != x):             # every candidate is +inf: argmin landed on a masked entry
            y = int(np.flatnonzero((size > 0) & (index != x))[0])
        dmin = D[x, y]
        if len(chain) > 1:
            p = chain[-2]
            if not (dmin < D[x, p]):                 # the previous element keeps a tie
                y, dmin = p, D[x, p]
        if len(chain) == 1 or y != chain[-2]:
            chain.append(y)
            continue
        chain.pop()
        chain.pop()
        a, b = min(x, y), max(x, y)
        na, nb = float(size[a]), float(size[b])
        k = (size > 0) & (index != a) & (index != b)
        new = _lance_williams(method, D[a, k], D[b, k], dmin, na, nb, size[k].astype(np.float64))
        D[b, k] = new
        D[k, b] = new
        size[b] += size[a]
        size[a] = 0
        merges.append((a, b))
        heights.append(dmin)
        sizes.append(size[b])
    return (np.asarray(merges, dtype=np.int64).reshape(-1, 2), np.asarray(heights, dtype=np.float64),
            np.asarray(sizes, dtype=np.int64))


def label(merges, heights, n):
    """scipy's / sklearn's children_: stable sort by height, merge i creates cluster n + i, each row (min, max) of the
    two roots."""
    order = np.argsort(heights, kind="stable")
    parent = list(range(2 * n - 1))

    def find(v):
        root = v
        while parent[root] != root:
            root = parent[root]
        while parent[v] != root:
            parent[v], v = root, parent[v]
        return root

    children = np.empty((n - 1, 2), dtype=np.int64)
    for i, m in enumerate(order):
        ra, rb = find(int(merges[m, 0])), find(int(merges[m, 1]))
        children[i] = (min(ra, rb), max(ra, rb))
        parent[ra] = parent[rb] = n + i
    return children, np.asarray(heights, dtype=np.float64)[order]


def linkage_ref(X, method="ward", metric="euclidean"):
    """(children [n-1, 2] int64, heights [n-1] fp64) of the fp32 matrix X."""
    X = np.asarray(X, dtype=np.float32)
    merges, heights, _ = nn_chain(pairwise(X, metric), method)
    return label(merges, heights, X.shape[0])


def smallest_relative_gap(heights):
    """min over consecutive sorted heights of (h[i+1] - h[i]) / h[i+1]: the condition of an exact comparison."""
    h = np.sort(np.asarray(heights, dtype=np.float64))
    if len(h) < 2:
        return np.inf
    gap = h[1:] - h[:-1]
    return float(np.min(np.where(gap > 0, gap / np.where(h[1:] > 0, h[1:], 1.0), 0.0)))


def check_dendrogram(children, n):
    """Every index 0 .. 2n-3 is a child exactly once, a child exists before its parent, and sizes add up to n."""
    children = np.asarray(children)
    assert children.shape == (n - 1, 2)
    assert sorted(children.ravel().tolist()) == list(range(2 * n - 2))
    size = [1] * n + [0] * (n - 1)
    for i, (a, b) in enumerate(children.tolist()):
        assert a < n + i and b < n + i and a != b
        size[n + i] = size[a] + size[b]
    assert size[2 * n - 2] == n
