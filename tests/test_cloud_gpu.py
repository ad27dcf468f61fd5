"""GPU tier: normals, tangent frames and gradient stencils of a point cloud (dn_cloud.hip) on the device -- the shared cases of
cloud_cases.py, one workload-sized cloud through ``geometry.cloud_operators`` and the point-cloud branch of ``compute_operators`` feeding a
DiffusionNet forward."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cloud_cases

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("N,k,seed,axes,noise", cloud_cases.CASES)
def test_case(dev, N, k, seed, axes, noise):
    cloud_cases.run_case(dev, N, k, seed, axes, noise)


def test_reference_fixture(dev):
    cloud_cases.run_reference_fixture(dev)


def test_single_point_is_rejected(dev):
    cloud_cases.run_single_point_is_rejected(dev)


def test_given_normals(dev):
    cloud_cases.run_given_normals(dev)


def test_sparse_operators_equal_the_raw_rows(dev):
    cloud_cases.run_sparse_equals_raw(dev)


def test_collinear_and_coincident_points(dev):
    cloud_cases.run_collinear(dev)


def test_duplicate_points(dev):
    cloud_cases.run_duplicates(dev)


def test_own_and_out_of_range_indices(dev):
    cloud_cases.run_bad_indices(dev)


def test_ops_validation(dev):
    cloud_cases.run_ops_validation(dev)


def test_abi_errors(dev):
    cloud_cases.run_abi_errors()


def test_workload_cloud_end_to_end(dev):
    """10 000 points, 30 neighbours: ``geometry.cloud_operators`` on the device against the host route in fp64, under the same checker."""
    import diffusion_net
    pts = cloud_cases.sample(10000, 7, (1.0, 0.7, 0.5), 0.002)     # (seed 7: among 10 000 points most seeds hold one whose 30th and 31st
    #                                                                 neighbours are closer than the kNN bound, which the checker refuses)
    truth = cloud_cases.truth_from_host_route(pts, 30)
    verts = torch.from_numpy(pts).to(dev)
    frames, gX, gY = diffusion_net.geometry.cloud_operators(verts, 30)
    assert frames.is_cuda and gX.is_cuda and gY.is_cuda and gX.is_coalesced() and gX._nnz() == 10000 * 31
    cloud_cases.check_cloud(pts, 30, cloud_cases.sparse_to_got(frames, gX, gY), truth, "workload_n10000_k30", dev)


def test_compute_operators_on_a_cloud_feeds_the_network(dev):
    """``compute_operators`` with empty faces on the device: the reference's seven-tuple, and a DiffusionNet forward on it that matches the
    oracle on the same operators within the margin of the single-mesh parity cases."""
    import diffusion_net
    import parity_cases
    from diffusion_net import synthetic
    from oracle import diffusionnet_oracle as orc
    N, K, C = 300, 16, 32
    pts = cloud_cases.sample(N, 3)
    v64 = torch.from_numpy(pts.astype(np.float64))
    nbr = diffusion_net.geometry.find_knn(v64, v64, 8, omit_diagonal=True, method="cpu_kd").indices.numpy()
    A = sp.coo_matrix((np.ones(N * 8), (np.repeat(np.arange(N), 8), nbr.reshape(-1))), shape=(N, N)).tocsr()
    A = ((A + A.T) > 0).astype(np.float64)                                  # a symmetric kNN-graph Laplacian, unit-sphere masses
    L, mass = (sp.diags(np.asarray(A.sum(axis=1)).reshape(-1)) - A).tocsr(), np.full(N, 4 * np.pi / N)
    verts = torch.from_numpy(pts).to(dev)
    out = diffusion_net.geometry.compute_operators(verts, torch.zeros(0, 3, dtype=torch.long, device=dev), K, laplacian=(L, mass))
    frames, massvec, Lt, evals, evecs, gX, gY = out
    assert len(out) == 7
    for t, shape in zip(out, ((N, 3, 3), (N,), (N, N), (K,), (N, K), (N, N), (N, N))):
        assert t.dtype == torch.float32 and t.device == verts.device and tuple(t.shape) == shape
    for m in (Lt, gX, gY):
        assert m.is_sparse and m.is_coalesced()
    assert gX._nnz() == N * 31

    torch.manual_seed(4)
    model = diffusion_net.layers.DiffusionNet(3, 6, C_width=C, N_block=2, outputs_at="vertices", dropout=False)
    model.load_state_dict(synthetic.randomize_times(model.state_dict(), seed=4))
    params = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(dev).eval()
    with torch.no_grad():
        got = model(verts, massvec, L=Lt, evals=evals, evecs=evecs, gradX=gX, gradY=gY)
    c = lambda t: t.cpu()
    ref = orc.net_forward(params, c(verts), c(massvec), c(evals), c(evecs), gradX=c(gX), gradY=c(gY), outputs_at="vertices")
    err = parity_cases.helpers.rel_max(got.cpu(), ref)
    parity_cases.helpers.record_margin("cloud_compute_operators_forward", dev, n=N, k_eig=K, fwd_rel_max=err, fwd_tol=parity_cases.FWD_TOL)
    assert tuple(got.shape) == (N, 6)
    assert err < parity_cases.FWD_TOL, err
