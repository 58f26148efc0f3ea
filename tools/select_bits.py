"""Raw outputs of searches that run every block-select site (flat with certificate failures and ties, filter-each lists around
k and with repeats, the IVF indexes of tests/test_ivf_select_edges_gpu.py), for a bit-for-bit comparison of two libraries:

    SQE_LIB=<library A> python tools/select_bits.py run a.npz
    SQE_LIB=<library B> python tools/select_bits.py run b.npz
    python tools/select_bits.py cmp a.npz b.npz      -> one line per array, `same` or `DIFFERS`

(The trained centroids differ between two runs of ONE library: k-means accumulates with fp32 atomics.)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

if sys.argv[1] == "cmp":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    bad = 0
    for name in a.files:
        same = a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes()
        print("same   " if same else "DIFFERS", name, a[name].shape)
        bad += not same
    print("arrays that differ:", bad, "of", len(a.files))
    sys.exit(0)

from semantic_query_engine_amd import Context, VectorIndex, INDEX_IVF_FLAT, _native
from tests import test_ivf_select_edges_gpu as E

dest = sys.argv[2]
out = {}
ctx = Context(0)
rng = np.random.default_rng(7)

# flat: certificate failures (a crowd of near-identical rows) -> collect_rescore_kernel; plain select_rescore_kernel; padding
x = rng.standard_normal((20000, 256)).astype(np.float32)
c = rng.standard_normal(256).astype(np.float32)
x[5000:8000] = c + 3e-3 * rng.standard_normal((3000, 256)).astype(np.float32)
x[9000:9400] = x[9000]                                  # 400 bit-identical rows
q = rng.standard_normal((64, 256)).astype(np.float32)
q[:16] = c + 1e-3 * rng.standard_normal((16, 256)).astype(np.float32)
q[16:20] = x[9000]
idx = VectorIndex(ctx, 256); idx.add(x)
ctx.stats_reset()
for k in (1, 10, 200):
    out[f"flat_cos_{k}"], out[f"flat_ids_{k}"] = idx.search(q, k)
out["flat_uncertified"] = np.array([ctx.stats()["uncertified"]])
small = VectorIndex(ctx, 256); small.add(x[:50])
out["small_cos"], out["small_ids"] = small.search(q, 100)
# filter_each: fewer than k, exactly k, more, repeats and dead ids
lists = [rng.integers(0, 20000, n) for n in (0, 5, 10, 11, 300, 1000, 5000)]
lists.append(np.concatenate([np.arange(9000, 9400), np.arange(9000, 9400), [-5, 10**9]]))
loq = (np.arange(64) % len(lists)).astype(np.int32)
for k in (10, 256):
    out[f"each_cos_{k}"], out[f"each_ids_{k}"] = idx.search_filtered_each(q, k, lists, loq)

def ivf(name, x, q, nlist, seed, cases, mutate=None):
    ix = E._index(ctx, x, nlist, seed)
    if mutate: mutate(ix, x, q)
    cen, assign = ix.ivf_export(nlist)
    out[f"{name}_cen"], out[f"{name}_assign"] = cen, assign
    for k, nprobe in cases:
        out[f"{name}_cos_{k}_{nprobe}"], out[f"{name}_ids_{k}_{nprobe}"] = ix.search(q, k, nprobe=nprobe)

def copies(n, d, m, seed):
    def f(ix, x, q):
        r = np.random.default_rng(seed)
        v = r.standard_normal(d).astype(np.float32)
        rows = r.permutation(n)[:m]
        x[rows] = v
        ix.update(rows, x[rows])
        q[:4] = v + 0.01 * r.standard_normal((4, d)).astype(np.float32)
    return f

x1, q1 = E._data(500, 64, 24, 101); ivf("small", x1, q1, 8, 102, [(10, 2), (60, 2), (256, 2)])
x2, q2 = E._data(6000, 64, 16, 111); ivf("fast", x2, q2, 8, 112, [(10, 4)])
x3, q3 = E._data(6000, 64, 16, 111); ivf("ties", x3, q3, 8, 112, [(10, 4), (60, 4)], copies(6000, 64, 2000, 113))
x4, q4 = E._data(3000, 64, 16, 121); ivf("dense", x4, q4, 128, 122, [(10, p) for p in (1, 8, 100, 120, 128)])
x5, q5 = E._data(2000, 256, 160, 131); ivf("colA", x5, q5, 4, 132, [(10, 4)])
x6, q6 = E._data(6000, 256, 80, 141); ivf("colB", x6, q6, 8, 142, [(10, 8), (64, 8)])
x7, q7 = E._data(6000, 256, 80, 141); ivf("colC", x7, q7, 8, 142, [(10, 8)], copies(6000, 256, 1500, 143))
np.savez(dest, **out)
print(dest, os.path.basename(_native.LIB_PATH), len(out), "arrays; uncertified", out["flat_uncertified"])
