"""Shared bodies of the farthest-point-sampling tests (drivers: test_fps_emu.py on the emulator build, test_fps_gpu.py on the device,
test_fps_host.py for the host routes of ``geometry.farthest_point_sampling``).

The yardstick is ``model``: the sampling loop in fp32 numpy, every product and sum rounded on its own --
d2 = (dx*dx + dy*dy) + dz*dz, min_d = d2 < min_d ? d2 : min_d, next sample = first index of the largest min_d, first sample = first index
of the smallest (x*x + y*y) + z*z.  Both kernel routes must reproduce its ``order``, ``radii`` and ``min_dist2`` BIT FOR BIT: there is no
tolerance anywhere in this file."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# clouds of at most threads * P points run in the instantiation (threads, P) of the resident kernel (dn_fps.hip); past the last, stepped
RESIDENT_STEPS = (64 * 8, 256 * 8, 1024 * 8)
RESIDENT_MAX = 1024 * 23
SLICE = 1024               # points per workgroup of the stepped route


def model(pts, n_sample, start=None):
    """(order [n_sample] int64, radii [n_sample] fp32, min_dist2 [N] fp32) of ONE cloud, pts [N, 3] fp32 already normalised."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    x, y, z = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
    if start is None:
        i = int(np.argmin((x * x + y * y) + z * z))
    else:
        i = int(start)
    md = np.full(len(x), np.inf, dtype=np.float32)
    order = np.zeros(n_sample, dtype=np.int64)
    radii = np.zeros(n_sample, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(n_sample):
            order[s] = i
            radii[s] = np.float32(np.inf) if s == 0 else md[i]
            dx, dy, dz = x - x[i], y - y[i], z - z[i]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            md = np.where(d2 < md, d2, md)
            i = int(np.argmax(md))
    return order, radii, md


def mask_of(order, n):
    m = np.zeros(n, dtype=bool)
    m[np.asarray(order).reshape(-1)] = True
    return m


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cloud(n, seed, kind="randn"):
    """A finite fp32 cloud, roughly inside the unit ball (``ops.fps`` takes its points as they are)."""
    rs = np.random.RandomState(seed)
    p = rs.randn(n, 3)
    if kind == "sphere":
        p /= np.linalg.norm(p, axis=1, keepdims=True)
    else:
        p *= 0.3
    return p.astype(np.float32)


def grid_cloud(shift=0):
    """8 x 8 x 8 lattice with coordinates (2 g - 7) * 2^(shift - 4): every difference, square and sum is exact in fp32, so whole shells of
    points tie exactly and only the lowest-index rule orders them."""
    g = (2.0 * np.arange(8) - 7.0) * 2.0 ** (shift - 4)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def _fps(dev, pts, n_sample, offsets=None, start=None, route=0):
    """``ops.fps`` on ``dev`` -> numpy (order, radii, min_dist2)."""
    from diffusion_net import ops
    st = None if start is None else torch.as_tensor(np.asarray(start, dtype=np.int64)).to(dev)
    o, r, m = ops.fps(torch.from_numpy(np.ascontiguousarray(pts)).to(dev), n_sample, offsets=offsets, start=st, route=route,
                      return_min_dist=True)
    assert o.dtype == torch.int64 and r.dtype == torch.float32 and m.dtype == torch.float32
    return o.cpu().numpy(), r.cpu().numpy(), m.cpu().numpy()


def check_single(dev, pts, n_sample, route, start=None):
    """One cloud on one route against the model, bit for bit; returns the kernel's triple."""
    want = model(pts, n_sample, start)
    o, r, m = _fps(dev, pts, n_sample, start=None if start is None else [start], route=route)
    assert o.shape == (1, n_sample) and r.shape == (1, n_sample) and m.shape == (len(pts),)
    assert same_bits(o[0], want[0]), ("order", len(pts), n_sample, route)
    assert same_bits(r[0], want[1]), ("radii", len(pts), n_sample, route)
    assert same_bits(m, want[2]), ("min_dist2", len(pts), n_sample, route)
    return o, r, m


def resident_sizes(on_gpu):
    sizes = [1, 2, 63, 64, 65]
    for n in RESIDENT_STEPS:
        sizes += [n, n + 1]
    return sizes + ([RESIDENT_MAX] if on_gpu else [])


def run_resident_size(dev, n):
    """One cloud size on the resident route: few samples at the big sizes (the point is which instantiation runs and its ragged tail)."""
    pts = cloud(n, 1000 + n)
    for k in sorted({1, min(2, n), min(n, 8 if n > 65 else n)}):
        check_single(dev, pts, k, 1)


def run_resident_rejects_past_capacity(dev):
    from diffusion_net import _hip
    assert _hip.FPS_RESIDENT_MAX_POINTS == RESIDENT_MAX == _hip.lib().dn_fps_resident_max_points()
    pts = torch.zeros(RESIDENT_MAX + 1, 3).to(dev)
    from diffusion_net import ops
    try:
        ops.fps(pts, 2, route=1)
    except ValueError:
        pass
    else:
        raise AssertionError("the resident route took a cloud past its capacity")


STEPPED_SIZES = (1, 5, SLICE, SLICE + 1, 2 * SLICE, 2 * SLICE + 452, 3 * SLICE)   # one slice, +1, two workgroups, three with a ragged last, three


def run_stepped_size(dev, n):
    pts = cloud(n, 2000 + n)
    for k in sorted({1, min(2, n), min(n, 7)}):
        check_single(dev, pts, k, 2)


def run_routes_agree(dev, n=1500, n_sample=40):
    """Both routes on the same input: the same bits, and the same bits twice."""
    pts = cloud(n, 31)
    a = check_single(dev, pts, n_sample, 1)
    b = check_single(dev, pts, n_sample, 2)
    for got in (check_single(dev, pts, n_sample, 1), check_single(dev, pts, n_sample, 2), _fps(dev, pts, n_sample, route=0)):
        for u, v, w in zip(a, b, got):
            assert same_bits(u, v) and same_bits(u, w)


def run_batch(dev, sizes, n_sample, route):
    """Clouds packed back to back: every cloud equals the model of that cloud alone (which the single-cloud tests tie to the kernel)."""
    clouds = [cloud(n, 3000 + i) for i, n in enumerate(sizes)]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    packed = np.concatenate(clouds)
    o, r, m = _fps(dev, packed, n_sample, offsets=offsets.tolist() if route else torch.from_numpy(offsets), route=route)   # (list or host tensor)
    assert o.shape == (len(sizes), n_sample)
    for c, pts in enumerate(clouds):
        want = model(pts, n_sample)
        assert same_bits(o[c] - offsets[c], want[0]) and same_bits(r[c], want[1]), (c, route)
        assert same_bits(m[offsets[c]:offsets[c + 1]], want[2]), (c, route)
    single = _fps(dev, clouds[-1], n_sample, route=route)
    assert same_bits(single[0][0], o[-1] - offsets[-2]) and same_bits(single[1][0], r[-1])


def run_no_clouds(dev):
    from diffusion_net import ops
    for route in (0, 1, 2):
        o, r, m = ops.fps(torch.zeros(0, 3).to(dev), 3, offsets=[0], route=route, return_min_dist=True)
        assert tuple(o.shape) == (0, 3) and tuple(r.shape) == (0, 3) and tuple(m.shape) == (0,)


def run_start(dev):
    """The first sample named by the caller (rows of the packed array), and left to the kernel."""
    pts = cloud(700, 41)
    for route in (1, 2):
        check_single(dev, pts, 20, route, start=123)
        check_single(dev, pts, 20, route, start=699)
        check_single(dev, pts, 20, route)
    sizes = [130, 90]
    clouds = [cloud(n, 42 + i) for i, n in enumerate(sizes)]
    for route in (0, 2):
        o, r, m = _fps(dev, np.concatenate(clouds), 10, offsets=[0, 130, 220], start=[5, 130 + 77], route=route)
        for c, (pts_c, st, off) in enumerate(zip(clouds, (5, 77), (0, 130))):
            want = model(pts_c, 10, st)
            assert same_bits(o[c] - off, want[0]) and same_bits(r[c], want[1])


def golden_cases():
    z = np.load(os.path.join(GOLDEN, "geom_fps_ref.npz"))
    for name in z["cases"]:
        name = str(name)
        yield name, z[name + "/points"], z[name + "/normalized"], int(z[name + "/n_sample"]), z[name + "/mask"], bool(z[name + "/gap_checked"])


def run_reference_fixture(dev):
    """``ops.fps`` on the reference's own normalised points reproduces the reference's mask, exact ties and duplicates included."""
    ran = 0
    for name, raw, normalized, n_sample, mask, _ in golden_cases():
        for route in (1, 2):
            o, r, m = _fps(dev, normalized, n_sample, route=route)
            assert np.array_equal(mask_of(o, len(normalized)), mask), (name, route)
        ran += 1
    assert ran == 4


def run_exact_ties(dev):
    """The lattice at three power-of-two scales: exact arithmetic, so the model and the kernels face the same ties."""
    for shift in (0, -3, 5):
        pts = grid_cloud(shift)
        a = check_single(dev, pts, 100, 1)
        b = check_single(dev, pts, 100, 2)
        assert same_bits(a[0], b[0])
        assert len(set(a[0][0].tolist())) == 100


def run_properties(dev):
    """radii never increases, radii[s] is the largest min_d after s samples, indices are distinct."""
    pts = cloud(600, 51, "sphere")
    for route in (1, 2):
        o, r, m = _fps(dev, pts, 64, route=route)
        o, r = o[0], r[0]
        assert np.isinf(r[0]) and bool((r[1:] <= r[:-1]).all())
        assert len(set(o.tolist())) == 64 and o.min() >= 0 and o.max() < 600
        md = np.full(600, np.inf, dtype=np.float32)
        for s in range(64):
            if s:
                assert md.max() == r[s] and int(np.argmax(md)) == o[s], s
            d = pts - pts[o[s]]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            md = np.minimum(md, d2)
        assert same_bits(md, m)
    dup = cloud(40, 52)
    dup[30:] = dup[:10]                       # 30 distinct points, 40 samples: all distinct while there are distinct points, then index 0 ... again
    for route in (1, 2):
        o, r, m = check_single(dev, dup, 40, route)
        assert len(set(o[0][:30].tolist())) == 30 and bool((r[0][30:] == 0).all()) and bool((m == 0).all())


def run_non_finite(dev):
    """One NaN and one inf planted in the middle cloud of three: the call returns, every index is inside its cloud, and the other clouds
    are bitwise what they are without it."""
    sizes = [200, 300, 150]
    offsets = [0, 200, 500, 650]
    clouds = [cloud(n, 60 + i) for i, n in enumerate(sizes)]
    clean = np.concatenate(clouds)
    dirty = clean.copy()
    dirty[200 + 17, 1] = np.nan
    dirty[200 + 203, 0] = np.inf
    for route in (0, 2):
        a = _fps(dev, clean, 50, offsets=offsets, route=route)
        b = _fps(dev, dirty, 50, offsets=offsets, route=route)
        for c in range(3):
            assert bool((b[0][c] >= offsets[c]).all()) and bool((b[0][c] < offsets[c + 1]).all()), (c, route)
        for c in (0, 2):
            assert same_bits(a[0][c], b[0][c]) and same_bits(a[1][c], b[1][c])
            assert same_bits(a[2][offsets[c]:offsets[c + 1]], b[2][offsets[c]:offsets[c + 1]])


def run_abi_errors():
    """Every non-zero return of dn_fps_f32, through ctypes, on host buffers: nothing is launched, the outputs keep their fill.  The
    workspace query is exact."""
    from diffusion_net import _hip
    L = _hip.lib()
    cap = L.dn_fps_resident_max_points()
    assert cap == RESIDENT_MAX
    n = 1500
    pts = torch.from_numpy(cloud(n, 71))
    offs = torch.tensor([0, n], dtype=torch.int64)
    order = torch.full((64,), -7, dtype=torch.int64)
    radii = torch.full((64,), -7.0)
    ws = torch.zeros(1 << 20, dtype=torch.uint8)

    def call(n_clouds=1, min_points=n, max_points=n, n_sample=5, route=0, ws_bytes=ws.numel()):
        return L.dn_fps_f32(pts.data_ptr(), offs.data_ptr(), n_clouds, min_points, max_points, n_sample, None, route, order.data_ptr(),
                            radii.data_ptr(), None, ws.data_ptr(), ws_bytes, None)

    assert call(n_sample=0) != 0                                   # n_sample < 1
    assert call(n_sample=n + 1) != 0                               # n_sample > min_points
    assert call(min_points=3, n_sample=4) != 0                     # (the smallest cloud decides)
    assert call(min_points=cap + 1, max_points=cap + 1, route=1) != 0   # resident route past the capacity
    assert call(route=3) != 0 and call(route=-1) != 0              # unknown route
    assert call(n_clouds=-1) != 0                                  # n_clouds < 0
    need = L.dn_fps_workspace_bytes(n, 1, n, 5, 2)
    assert need >= n * 4 and L.dn_fps_workspace_bytes(n, 1, n, 5, 1) == 0 and L.dn_fps_workspace_bytes(n, 1, n, 5, 0) == 0
    assert L.dn_fps_workspace_bytes(cap + 1, 1, cap + 1, 5, 0) > 0  # the library's choice past the capacity is the stepped route
    assert call(route=2, ws_bytes=need - 1) != 0                   # workspace smaller than the query says
    assert bool((order == -7).all()) and bool((radii == -7.0).all())
    assert call(n_clouds=0) == 0                                   # no cloud: success, nothing launched
    assert bool((order == -7).all()) and bool((radii == -7.0).all())
    assert call(route=2, ws_bytes=need) == 0                       # and the exact size is enough
    want = model(pts.numpy(), 5)
    assert same_bits(order[:5].numpy(), want[0]) and same_bits(radii[:5].numpy(), want[1])
    assert bool((order[5:] == -7).all())
