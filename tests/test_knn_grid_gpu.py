"""GPU tier: the cell-grid k-nearest-neighbour search (dn_knn_grid.hip) on the device -- the shared cases of knn_grid_cases.py against
``ops.knn`` bit for bit and against fp64 brute force, a 3 000-point sphere, the routing of ``geometry.find_knn(method='grid')`` and of the
point-cloud pipeline, graph capture and the registered operator under ``torch.compile``."""
import os

import pytest
import torch

import knn_cases
import knn_grid_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    from diffusion_net import _hip
    _hip._use_library_for_tests(None, False)
    if not os.path.exists(_hip.LIB_PATH):  # fresh checkout on the GPU box: compile the HIP sources
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.lib()                      # raises if libdiffnet_hip.so is missing: no fallback
    assert lib.dn_knn_grid_cell_budget() > 0
    return torch.device("cuda:0")


@pytest.mark.parametrize("N,M,D,k,flags", knn_grid_cases.CASES)
def test_case(dev, N, M, D, k, flags):
    knn_grid_cases.run_case(dev, N, M, D, k, flags)


def test_exact_ties(dev):
    knn_grid_cases.run_exact_ties(dev)


def test_duplicates_zero_extent_and_collinear(dev):
    knn_grid_cases.run_duplicates(dev)


def test_clusters_and_outlier_close_without_a_scan(dev):
    knn_grid_cases.run_clusters(dev)


def test_cross_query_scans(dev):
    knn_grid_cases.run_cross(dev)


def test_second_run_gives_the_same_bits(dev):
    knn_grid_cases.run_repeat(dev)


def test_pipeline_routes_agree(dev, monkeypatch):
    knn_grid_cases.run_pipeline(dev, monkeypatch)


def test_sphere_3000(dev):
    """3 000 points on the unit sphere, k = 30, the pipeline's self-query: ops.knn's bits, right against fp64 on the device, no scan."""
    from diffusion_net import ops
    g = torch.Generator().manual_seed(41)
    pts = torch.nn.functional.normalize(torch.randn(3000, 3, generator=g), dim=1).to(dev)
    dist, idx, info = ops.knn_grid(pts, pts, 30, omit_diagonal=True, return_info=True)
    want = ops.knn(pts, pts, 30, omit_diagonal=True)
    assert torch.equal(idx, want[1]) and torch.equal(dist, want[0])
    print("knn_grid sphere 3000:", info)
    assert info["full_scans"] == 0
    knn_cases.check_knn_on_device(pts, pts, 30, False, True, (dist, idx))


def test_find_knn_routing(dev):
    import diffusion_net
    from diffusion_net import ops
    src, tgt = knn_cases.inputs(300, 400, 3, False, 42)
    src, tgt = src.to(dev), tgt.to(dev)
    want = ops.knn_grid(src, tgt, 7)
    got = diffusion_net.find_knn(src, tgt, 7, method="grid")
    assert torch.equal(got.values, want[0]) and torch.equal(got.indices, want[1])
    got = diffusion_net.find_knn(src, src, 7, omit_diagonal=True, method="grid")
    want = ops.knn_grid(src, src, 7, omit_diagonal=True)
    assert torch.equal(got.values, want[0]) and torch.equal(got.indices, want[1])
    # where the grid kernel does not apply, 'grid' is 'brute'
    a30, b30 = knn_cases.inputs(200, 300, 30, False, 43)
    for a, b, k in ((a30.to(dev), b30.to(dev), 5), (src, tgt, 40), (src.cpu(), tgt.cpu(), 5), (src.double(), tgt.double(), 5)):
        got = diffusion_net.find_knn(a, b, k, method="grid")
        want = diffusion_net.find_knn(a, b, k, method="brute")
        assert torch.equal(got.values, want.values) and torch.equal(got.indices, want.indices)
    with pytest.raises(ValueError, match="unrecognized method"):
        diffusion_net.find_knn(src, tgt, 3, method="ball_tree")
    with pytest.raises(ValueError, match="largest"):
        diffusion_net.find_knn(src, tgt, 3, largest=True, method="grid")
    with pytest.raises(ValueError):
        ops.knn_grid(a30.to(dev), b30.to(dev), 3)          # D > 3


def test_graph_capture_replays_the_eager_bits(dev):
    from diffusion_net import ops
    src, tgt = knn_cases.inputs(700, 900, 3, False, 44)
    src, tgt = src.to(dev), tgt.to(dev)
    eager = ops.knn_grid(src, tgt, 12)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.knn_grid(src, tgt, 12)                         # warm-up off the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.knn_grid(src, tgt, 12)
    out[0].zero_(); out[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


def test_registered_operator_under_torch_compile(dev):
    from diffusion_net import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.knn_grid)
    src, tgt = knn_cases.inputs(300, 400, 3, False, 45)
    src, tgt = src.to(dev), tgt.to(dev)

    def f(a, b):
        d, i = torch.ops.diffusion_net.knn_grid(a * 1.0, b, 4, False, 0)
        return d + 0.0, i

    eager = f(src, tgt)
    compiled = torch.compile(f, fullgraph=True)(src, tgt)
    assert torch.equal(compiled[0], eager[0]) and torch.equal(compiled[1], eager[1])
    knn_cases.check_knn(src.cpu(), tgt.cpu(), 4, False, False, eager)
