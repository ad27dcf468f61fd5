"""GPU tier: the local-Delaunay Laplacian and mass of a point cloud (dn_cloud_lap.hip) on the device -- the shared cases of
cloud_lap_cases.py, ``compute_operators(..., laplacian="delaunay")`` without the host feeding a DiffusionNet forward + backward, and the
device steps captured in a HIP graph."""
import os

import numpy as np
import pytest
import torch

import cloud_lap_cases

pytestmark = pytest.mark.gpu

NO_FACES = torch.zeros(0, 3, dtype=torch.long)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    from diffusion_net import _hip
    _hip._use_library_for_tests(None, False)
    if not os.path.exists(_hip.LIB_PATH):  # fresh checkout on the GPU box: compile the HIP sources
        import __graft_entry__
        __graft_entry__.build()
    _hip.lib()                            # raises if libdiffnet_hip.so is missing: no fallback
    return torch.device("cuda:0")


@pytest.mark.parametrize("n,k,seed,kind", cloud_lap_cases.CASES)
def test_case(dev, n, k, seed, kind):
    cloud_lap_cases.run_case(dev, n, k, seed, kind)


def test_one_neighbour_gives_no_triangle(dev):
    cloud_lap_cases.run_k1(dev)


def test_two_neighbours(dev):
    cloud_lap_cases.run_k2(dev)


def test_given_frames(dev):
    cloud_lap_cases.run_given_frames(dev)


@pytest.mark.parametrize("name", cloud_lap_cases.DEGENERATE)
def test_degenerate_input(dev, name):
    cloud_lap_cases.run_degenerate(dev, name)


def test_own_and_out_of_range_indices(dev):
    cloud_lap_cases.run_bad_indices(dev)


def test_ops_validation(dev):
    cloud_lap_cases.run_ops_validation(dev)


def test_sparse_laplacian_equals_the_raw_csr(dev):
    cloud_lap_cases.run_sparse_equals_raw(dev)


def test_abi_errors(dev):
    cloud_lap_cases.run_abi_errors()


@pytest.fixture(scope="module")
def device_operators(dev):
    import diffusion_net
    pts = cloud_lap_cases.sample(300, 3)
    verts = torch.from_numpy(pts).to(dev)
    return pts, verts, diffusion_net.geometry.compute_operators(verts, NO_FACES.to(dev), 8, laplacian="delaunay")


def test_compute_operators_delaunay_stays_on_the_device(dev, device_operators):
    """Every output on the device; eigenvalues as the host route's (the two L differ by fp32 rounding, 1e-7, and eigsh runs to its own
    tolerance): rtol 1e-4, where the eigenvalue 0 of the constants is held to 1e-4 of the first non-zero one (a relative bound on a value
    that is zero up to the shift has no meaning); eigenvectors orthonormal in the mass to 1e-4."""
    import diffusion_net
    pts, verts, out = device_operators
    frames, massvec, L, evals, evecs, gX, gY = out
    N, K = 300, 8
    assert len(out) == 7
    for t, shape in zip(out, ((N, 3, 3), (N,), (N, N), (K,), (N, K), (N, N), (N, N))):
        assert t.dtype == torch.float32 and t.device == verts.device and tuple(t.shape) == shape
    for m in (L, gX, gY):
        assert m.is_sparse and m.is_coalesced()
    host = diffusion_net.geometry.compute_operators(torch.from_numpy(pts), NO_FACES, K, laplacian="delaunay")
    ev, ev_host = evals.cpu().double().numpy(), host[3].double().numpy()
    print("delaunay operators: device evals %s, host evals %s" % (ev, ev_host))
    assert np.allclose(ev[1:], ev_host[1:], rtol=1e-4, atol=0.0)
    assert abs(ev[0] - ev_host[0]) <= 1e-4 * ev_host[1]
    e, m = evecs.cpu().double(), massvec.cpu().double()
    assert torch.allclose(e.T @ (m[:, None] * e), torch.eye(K, dtype=torch.float64), atol=1e-4)
    assert abs(float(m.sum()) / (4 * np.pi) - 1.0) < 0.1


def test_delaunay_operators_feed_a_forward_and_backward(dev, device_operators):
    import diffusion_net
    from diffusion_net import synthetic
    _, verts, (frames, massvec, L, evals, evecs, gX, gY) = device_operators
    torch.manual_seed(4)
    model = diffusion_net.layers.DiffusionNet(3, 6, C_width=32, N_block=2, outputs_at="vertices", dropout=False)
    model.load_state_dict(synthetic.randomize_times(model.state_dict(), seed=4))
    model.to(dev).train()
    got = model(verts, massvec, L=L, evals=evals, evecs=evecs, gradX=gX, gradY=gY)
    assert tuple(got.shape) == (300, 6) and bool(torch.isfinite(got).all())
    got.square().mean().backward()
    grads = [p.grad for p in model.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)


def test_device_steps_replay_in_a_graph(dev):
    """Star, emit, the two stable sorts and the segment sums captured in one HIP graph (``ops._cloud_laplacian_launch``: everything
    ``ops.cloud_laplacian`` does short of its one host read of the status word and the entry count, which no graph can hold) and replayed
    twice: identical bits, and those of the eager call."""
    from diffusion_net import ops
    t, nbr, fr = cloud_lap_cases.inputs(dev, cloud_lap_cases.sample(300, 3), 16)
    eager = [x.clone() for x in ops._cloud_laplacian_launch(t, nbr, fr)]
    nnz = int(eager[5].item())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops._cloud_laplacian_launch(t, nbr, fr)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = ops._cloud_laplacian_launch(t, nbr, fr)
    runs = []
    for _ in range(2):
        for x in outs:
            x.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        runs.append([x.clone() for x in outs])
    for a, b, e, trim in zip(runs[0], runs[1], eager, (False, False, True, True, False, False, False)):
        if trim:
            a, b, e = a[:nnz], b[:nnz], e[:nnz]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), e.view(torch.int32))
    assert nnz > 0 and int(runs[0][6].item()) == 0
