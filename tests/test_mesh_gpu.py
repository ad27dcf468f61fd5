"""GPU tier: the operators of a triangle mesh (dn_mesh.hip) on the device -- the shared cases of mesh_cases.py,
``compute_operators_via(..., assembly="device")`` feeding a DiffusionNet forward + backward, and the device steps captured in a HIP graph."""
import os

import pytest
import torch

import mesh_cases

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


@pytest.mark.parametrize("name", mesh_cases.CASES + mesh_cases.DEGENERATE + mesh_cases.FALLBACK)
def test_case(dev, name):
    mesh_cases.check(dev, name)


@pytest.mark.parametrize("name", mesh_cases.CASES + mesh_cases.DEGENERATE + mesh_cases.FALLBACK)
def test_mesh_operators(dev, name):
    mesh_cases.check_mesh_operators(dev, name)


def test_empty_inputs(dev):
    mesh_cases.run_empty(dev)


def test_out_of_range_indices(dev):
    mesh_cases.run_bad_indices(dev)


def test_ops_validation(dev):
    mesh_cases.run_ops_validation(dev)


def test_abi_errors(dev):
    mesh_cases.run_abi_errors()


def test_custom_operators_are_registered_with_fake_kernels(dev):
    mesh_cases.run_library_ops(dev)


@pytest.fixture(scope="module")
def device_operators(dev):
    return mesh_cases.run_compute_operators(dev, None)


def test_compute_operators_with_device_assembly(dev, device_operators):
    assert all(t.is_cuda for t in device_operators)


def test_compute_operators_with_device_assembly_and_the_subspace_solver(dev):
    mesh_cases.run_compute_operators(dev, "subspace")


def test_device_operators_feed_a_forward_and_backward(dev, device_operators):
    import numpy as np
    verts = torch.from_numpy(np.array(mesh_cases.sphere300()[0])).to(dev)
    mesh_cases.run_forward_backward(dev, device_operators, verts)


def test_cache_round_trip_and_bad_values(dev, tmp_path):
    mesh_cases.run_cache_round_trip(dev, tmp_path)


def test_device_steps_replay_in_a_graph(dev):
    """Emit, the two stable sorts, the segment sums (``ops._mesh_assemble_launch``: everything ``ops.mesh_assemble`` does short of its one
    host read of the status word and the entry count, which no graph can hold), the normalisation of the normal sums and the vertex pass
    on the full-length column buffer, captured in one HIP graph on a single stream and replayed twice: identical bits, and those of the
    eager calls.

    (The outputs are filled with -3 before each replay, so the device has queued work when the graph starts: with the status words zeroed
    by hipMemsetAsync the word of the vertex pass read 0xC9C9C9C9 after the second replay; dn_mesh.hip zeroes with a kernel.)"""
    from diffusion_net import ops
    tv, tf = mesh_cases.tensors(dev, "sphere200")

    def steps():
        rowptr, col, lval, vrec, count, status = ops._mesh_assemble_launch(tv, tf)
        nsum = vrec[:, 1:]
        normals = (nsum / torch.linalg.vector_norm(nsum, dim=1, keepdim=True)).contiguous()
        frames, gx, gy, vstatus = ops._mesh_frames_gradients_launch(tv, rowptr, col, normals)
        return rowptr, col, lval, vrec, count, status, frames, gx, gy, vstatus

    eager = [x.clone() for x in steps()]
    nnz = int(eager[4].item())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            steps()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = steps()
    runs = []
    for _ in range(2):
        for x in outs:
            x.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        runs.append([x.clone() for x in outs])
    names = ("rowptr", "col", "lval", "vrec", "count", "status", "frames", "gx", "gy", "vertex status")
    assert nnz > 0 and [int(r[4].item()) for r in runs] == [nnz, nnz], (nnz, [int(r[4].item()) for r in runs])
    for name, a, b, e in zip(names, runs[0], runs[1], eager):
        if name in ("col", "lval", "gx", "gy"):                  # (behind the matrix the buffers are scratch)
            a, b, e = a[:nnz], b[:nnz], e[:nnz]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s differs between two replays" % name
        assert torch.equal(a.view(torch.int32), e.view(torch.int32)), "%s of the replays differs from the eager call's" % name
    assert int(runs[0][5].item()) == 0 and int(runs[0][9].item()) == 0
    want = ops.mesh_assemble(tv, tf)
    assert torch.equal(runs[0][2][:nnz], want[2]) and torch.equal(runs[0][1][:nnz], want[1])
