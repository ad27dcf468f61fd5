"""Shared bodies of the k-nearest-neighbour tests (drivers: test_knn_emu.py on the emulator build, test_knn_gpu.py on the device,
test_knn_host.py for the host routes of ``geometry.find_knn``).

The checker compares against fp64 brute force.  Its one tolerance is the a-priori bound of the difference form in fp32 -- one rounded
difference, D squares, D - 1 additions and one square root per distance: |dist - d64| <= (D + 4) * 2^-24 * d64.  It is derived, not tuned."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (N, M, D, k, flags): the smallest shapes at which the kernel can still go wrong
CASES = [
    (130, 77, 33, 1, ""),           # k = 1 path; M below one target tile; D no multiple of the chunk; ragged last query tile
    (200, 333, 3, 30, ""),          # several target tiles
    (200, 333, 30, 30, ""),         # (one chunk of 30 dimensions)
    (150, 200, 1, 5, ""),           # D = 1
    (257, 257, 3, 32, "omit"),      # k at the limit; diagonal excluded across tile borders
    (40, 40, 3, 39, "omit"),        # k = M - 1: every list fills exactly (39 is past the kernel's k <= 32: see run_case)
    (50, 9, 4, 9, ""),              # k = M
    (1, 1, 3, 1, ""),               # smallest possible input
    (200, 333, 30, 3, "largest"),   # largest-k ordering
    (100, 150, 70, 7, ""),          # several D chunks on the list path (the kernel stages 32 dimensions at a time: 32 + 32 + 6)
]
SPLITS = (1, 3, 0, 1000)


def rel_bound(D):
    return (D + 4) * 2.0 ** -24


def inputs(N, M, D, same, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(N, D, generator=g)
    tgt = src.clone() if same else torch.randn(M, D, generator=g)
    return src, tgt


def d64_matrix(src, tgt):
    a, b = src.detach().double().cpu(), tgt.detach().double().cpu()
    return (a[:, None, :] - b[None, :, :]).pow(2).sum(-1).sqrt()


def check_knn(src, tgt, k, largest, omit_diagonal, got, max_skipped=0.01, d64=None, row0=0):
    """Items 1-4 of the checker; returns the share of index positions that were too close to a neighbouring order statistic to be pinned.
    ``d64``: the fp64 distance block of these rows where the caller has it already (it may live on a device: the check then runs there);
    ``row0``: the index of the first row in the whole problem, which is where its diagonal lies."""
    where = d64.device if d64 is not None else torch.device("cpu")
    dist, idx = got[0].detach().to(where), got[1].detach().to(where)
    N, M, D = src.shape[0], tgt.shape[0], src.shape[1]
    rows = torch.arange(N, device=where)
    # 1. shapes, dtypes, index range, no repeats, no diagonal, monotone rows
    assert tuple(dist.shape) == (N, k) and tuple(idx.shape) == (N, k)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64
    if N == 0:
        return 0.0
    assert int(idx.min()) >= 0 and int(idx.max()) < M
    srt = idx.sort(dim=1).values
    assert not bool((srt[:, 1:] == srt[:, :-1]).any()), "an index is repeated within a row"
    if omit_diagonal:
        assert not bool((idx == (rows + row0)[:, None]).any()), "the diagonal was returned"
    step = dist[:, 1:] - dist[:, :-1]
    assert bool((step <= 0).all() if largest else (step >= 0).all()), "distances are not monotone along a row"
    if d64 is None:
        d64 = d64_matrix(src, tgt)
    rb = rel_bound(D)
    # 2. each returned distance is the distance of the returned pair
    pair = d64.gather(1, idx)
    err = (dist.double() - pair).abs()
    print("knn check N=%d M=%d D=%d k=%d: max |dist - d64| / d64 = %.3e (bound %.3e)" % (
        N, M, D, k, float((err / pair.clamp_min(1e-300)).max()), rb))
    assert bool((err <= rb * pair).all()), "a returned distance is not the distance of its pair"
    # 3. the row is the true top-k
    key = -d64 if largest else d64.clone()
    if omit_diagonal:
        key[rows, rows + row0] = float("inf")
    order = torch.argsort(key, dim=1, stable=True)[:, :min(k + 1, M)]
    stats = key.gather(1, order)
    true = stats[:, :k].abs()
    assert bool(((dist.double() - true).abs() <= rb * true).all()), "a row is not the true top-k"
    # 4. indices wherever the fp64 gaps to both neighbouring order statistics exceed twice the bound
    inf = torch.full((N, 1), float("inf"), dtype=torch.float64, device=where)
    nxt = torch.cat([stats[:, 1:], inf], dim=1)[:, :k]
    gap_next = nxt - stats[:, :k]
    gap_prev = torch.cat([inf, stats[:, 1:k] - stats[:, :k - 1]], dim=1)
    pinned = (gap_next > 2 * rb * true) & (gap_prev > 2 * rb * true)
    skipped = 1.0 - float(pinned.double().mean())
    print("knn check: %.4f %% of index positions skipped as near-ties" % (100 * skipped))
    assert skipped <= max_skipped, "too many near-ties for the index check to mean anything: %.3f" % skipped
    assert bool((idx[pinned] == order[:, :k][pinned]).all()), "an index differs from the fp64 argsort at a position with a clear gap"
    return skipped


def check_knn_on_device(src, tgt, k, largest, omit_diagonal, got, rows_per_block=1024):
    """The same checker against fp64 brute force computed on the tensors' device, a block of rows at a time (workload-sized inputs)."""
    s64, t64 = src.double(), tgt.double()
    worst = 0.0
    for r0 in range(0, src.shape[0], rows_per_block):
        r1 = min(r0 + rows_per_block, src.shape[0])
        d64 = torch.cdist(s64[r0:r1], t64, compute_mode="donot_use_mm_for_euclid_dist")
        worst = max(worst, check_knn(src[r0:r1], tgt, k, largest, omit_diagonal, (got[0][r0:r1], got[1][r0:r1]), d64=d64, row0=r0))
    return worst


def _knn(dev, src, tgt, k, largest=False, omit=False, n_split=0):
    from diffusion_net import ops
    d, i = ops.knn(src.to(dev), tgt.to(dev), k, largest=largest, omit_diagonal=omit, n_split=n_split)
    return d.cpu(), i.cpu()


def run_case(dev, N, M, D, k, flags, seed=0):
    """One row of the case table on the kernel, checked against fp64 brute force."""
    omit, largest = flags == "omit", flags == "largest"
    src, tgt = inputs(N, M, D, omit, 100 + seed)
    if k > 32:
        # k = M - 1 = 39 is past the kernel's limit (DN_KNN_MAX_K = 32).  The case runs as stated through the public entry point, whose
        # routing sends k > 32 to the torch path; the kernel refuses it; and the edge it names -- every list fills exactly -- is reached on the
        # kernel by the largest legal analogue, the first 33 points with k = 32.
        from diffusion_net import geometry, ops
        try:
            ops.knn(src.to(dev), tgt.to(dev), k, omit_diagonal=omit)
        except ValueError:
            pass
        else:
            raise AssertionError("k = %d was accepted by the kernel entry point" % k)
        got = geometry.find_knn(src.to(dev), tgt.to(dev), k, omit_diagonal=omit)
        check_knn(src, tgt, k, largest, omit, (got.values, got.indices))
        src, tgt, k = src[:33].contiguous(), tgt[:33].contiguous(), 32
    check_knn(src, tgt, k, largest, omit, _knn(dev, src, tgt, k, largest, omit))


def run_splits(dev, D, k, largest):
    """200 x 333: one slice, three, the library's choice and a clamped 1000 are the same bits, and right."""
    src, tgt = inputs(200, 333, D, False, 7)
    outs = [_knn(dev, src, tgt, k, largest, False, ns) for ns in SPLITS]
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    check_knn(src, tgt, k, largest, False, outs[0])


def lattice_expected(pts, k, largest, omit):
    """Stable argsort of (integer d^2, index) in int64."""
    p = pts.to(torch.int64)
    d2 = (p[:, None, :] - p[None, :, :]).pow(2).sum(-1)
    key = -d2 if largest else d2.clone()
    if omit:
        key[torch.arange(len(p)), torch.arange(len(p))] = torch.iinfo(torch.int64).max
    order = torch.argsort(key, dim=1, stable=True)[:, :k]
    return d2.gather(1, order), order


def run_exact_ties(dev):
    """Integer lattice points of {0,1,2,3}^3: every squared distance is an exact small integer, so the lower-index rule is all that orders ties."""
    g = torch.Generator().manual_seed(5)
    pts = torch.randint(0, 4, (150, 3), generator=g).float()
    for largest, omit, ns in ((False, False, 0), (False, True, 0), (True, False, 0), (False, False, 3), (True, True, 3), (False, True, 1)):
        d2, want = lattice_expected(pts, 8, largest, omit)
        dist, idx = _knn(dev, pts, pts, 8, largest, omit, ns)
        assert torch.equal(idx, want), (largest, omit, ns)
        exact = d2.double().sqrt()             # d^2 is exact here: what is left is the one square root, well inside the checker's bound
        assert bool(((dist.double() - exact).abs() <= rel_bound(3) * exact).all()), (largest, omit, ns)
    d2, want = lattice_expected(pts, 1, False, True)       # the k = 1 path merges sixteen threads' minima: same rule
    for ns in (0, 2):
        assert torch.equal(_knn(dev, pts, pts, 1, False, True, ns)[1], want)
    d2, want = lattice_expected(pts, 1, True, False)
    assert torch.equal(_knn(dev, pts, pts, 1, True, False, 0)[1], want)


def run_duplicates(dev):
    """Every point present twice, omit_diagonal, k = 1: the neighbour is the twin at distance 0, never the point itself."""
    g = torch.Generator().manual_seed(6)
    half = torch.randn(90, 3, generator=g)
    pts = torch.cat([half, half])
    for ns in (0, 2):
        dist, idx = _knn(dev, pts, pts, 1, False, True, ns)
        twin = (torch.arange(180) + 90) % 180
        assert torch.equal(idx[:, 0], twin) and bool((dist == 0).all())


def golden_cases():
    z = np.load(os.path.join(GOLDEN, "geom_knn_ref.npz"))
    for name in z["cases"]:
        name = str(name)
        k, largest, omit = (int(v) for v in z[name + "/k_largest_omit"])
        ref = {m: (torch.from_numpy(z["%s/%s_values" % (name, m)]), torch.from_numpy(z["%s/%s_indices" % (name, m)]))
               for m in ("brute", "cpu_kd") if "%s/%s_values" % (name, m) in z.files}
        yield name, torch.from_numpy(z[name + "/src"]), torch.from_numpy(z[name + "/tgt"]), k, bool(largest), bool(omit), ref


def check_against_reference(src, tgt, k, largest, omit, got, ref):
    """The reference's recorded outputs: equal indices (the inputs have no near-ties: asserted as in checker item 4, with no position
    skipped), distances within the bound."""
    skipped = check_knn(src, tgt, k, largest, omit, got)
    assert skipped == 0.0, "the fixture's inputs were chosen without near-ties"
    rb = rel_bound(src.shape[1])
    for method, (vals, inds) in ref.items():
        assert torch.equal(got[1].cpu(), inds), method
        err = (got[0].cpu().double() - vals.double()).abs() / vals.double().clamp_min(1e-300)
        print("knn fixture %s: max |dist - reference| / reference = %.3e (bound %.3e)" % (method, float(err.max()), rb))
        assert bool((err <= rb).all()), method


def run_reference_fixture(dev):
    """Device results on the fixture's inputs against the reference's recorded outputs."""
    for name, src, tgt, k, largest, omit, ref in golden_cases():
        check_against_reference(src, tgt, k, largest, omit, _knn(dev, src, tgt, k, largest, omit), ref)


def run_abi_errors():
    """Every non-zero return of dn_knn_f32, through ctypes, on host buffers: nothing is launched, dist / idx keep their fill."""
    from diffusion_net import _hip
    L = _hip.lib()
    assert L.dn_knn_max_k() == 32 == _hip.KNN_MAX_K
    src, tgt = inputs(70, 70, 3, False, 1)
    other = torch.randn(50, 3)
    dist = torch.full((70, 40), -7.0)
    idx = torch.full((70, 40), -7, dtype=torch.int64)
    ws = torch.zeros(1 << 20, dtype=torch.uint8)

    def call(s, t, dim, k, largest=0, omit=0, n_split=0, ws_bytes=ws.numel()):
        return L.dn_knn_f32(s.data_ptr(), s.shape[0], t.data_ptr(), t.shape[0], dim, k, largest, omit, n_split, dist.data_ptr(),
                            idx.data_ptr(), ws.data_ptr(), ws_bytes, None)

    assert call(src, tgt, 3, 0) != 0                      # k < 1
    assert call(src, tgt, 3, 33) != 0                     # k > dn_knn_max_k()
    assert call(src, other, 3, 32) == 0 and call(src, other[:31], 3, 32) != 0   # k > n_tgt
    dist.fill_(-7.0); idx.fill_(-7)
    assert call(src[:20], tgt[:20], 3, 20, omit=1) != 0   # k > n_tgt - 1 with the diagonal left out
    assert call(src, tgt, 0, 1) != 0                      # dim < 1
    assert call(src, other, 3, 1, omit=1) != 0            # omit_diagonal with n_src != n_tgt
    need = L.dn_knn_workspace_bytes(70, 70, 3, 5, 2)
    assert need >= 2 * 5 * 70 * 8
    assert call(src, tgt, 3, 5, n_split=2, ws_bytes=need - 1) != 0   # workspace smaller than the query says
    assert L.dn_knn_workspace_bytes(70, 70, 3, 5, 1) == 0
    assert bool((dist == -7.0).all()) and bool((idx == -7).all())
    assert call(src[:0], tgt, 3, 5) == 0                  # n_src == 0: success, nothing launched
    assert bool((dist == -7.0).all()) and bool((idx == -7).all())
    assert call(src, tgt, 3, 5, n_split=2, ws_bytes=need) == 0       # and the exact size is enough
    check_knn(src, tgt, 5, False, False, (dist.flatten()[:350].reshape(70, 5).clone(), idx.flatten()[:350].reshape(70, 5).clone()))
