"""Shared bodies of tests/test_hbits_emu.py (emulator build) and tests/test_hbits_gpu.py (device): the sign-bit words of the hidden
activations (dn_block_saved_t.hbits, include/diffnet_hip.h) that the block forward leaves for the chained backward.  Everything here is an
EQUALITY -- the words restate a predicate on values the forward stores, and the backward evaluates the same predicate from either source --
so no case carries a tolerance.  One DiffusionNetBlock through ops.block_fwd / ops.block_bwd (the plain launch functions under autograd)."""
import contextlib
import ctypes

import torch

import parity_cases
from diffusion_net import _hip, ops, synthetic

SIZES = ((5,), (16,), (17, 47), (300, 140, 131))      # rows below one 16-row half, an exact half, tiles straddling mesh ends and the batch end
K_CHAIN_BWD = 6                                       # dn_prof kind of chain_bwd_kernel
NO_CHAIN = 1                                          # DN_BLOCK_NO_CHAIN


@contextlib.contextmanager
def options(**kw):
    old = {k: _hip.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            _hip.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            _hip.set_option(k, v)


def make_mesh(V, K, seed):
    """synthetic.make_mesh_operators where it applies (V >= 16 and V >= K); below that a mesh of the same make on a ring: every vertex differences
    its four nearest ring neighbours, the eigenbasis is padded with zero columns (a mesh cannot have more modes than vertices)"""
    if V >= 16 and V >= K:
        return synthetic.make_mesh_operators(V, K, seed=seed)
    g = torch.Generator().manual_seed(seed)
    mass = (0.5 + torch.rand(V, generator=g)) * (12.566 / V)
    q, _ = torch.linalg.qr(torch.randn(V, min(V, K), generator=g))
    evecs = torch.zeros(V, K)
    evecs[:, :q.shape[1]] = q / mass.sqrt()[:, None]
    evals = torch.sort(torch.rand(K, generator=g)).values * (0.55 * K)
    evals[0] = 0.0
    v = torch.arange(V)
    cols = torch.stack([v, (v + 1) % V, (v - 1) % V, (v + 2) % V, (v - 2) % V], 1)
    idx = torch.stack([v[:, None].expand(V, 5).reshape(-1), cols.reshape(-1)], 0)
    ops_ = []
    for _ in range(2):
        off = torch.randn(V, 4, generator=g) * (0.1 * V ** 0.5)
        ops_.append(torch.sparse_coo_tensor(idx, torch.cat([-off.sum(1, keepdim=True), off], 1).reshape(-1), (V, V)).coalesce())
    return {"mass": mass, "evals": evals, "evecs": evecs, "gradX": ops_[0], "gradY": ops_[1]}


class Block:
    """Operands of one block call on a ragged synthetic batch: gather form (K as given, no spectral operands used) or spectral form (K = 128)."""

    def __init__(self, device, sizes, C, n_mlp, K, seed=3):
        meshes = [make_mesh(v, K, seed + i) for i, v in enumerate(sizes)]
        self.mb = parity_cases.pack(meshes, device, chunk_rows=64)
        self.V, self.C, self.n_mlp, self.device = sum(sizes), C, n_mlp, device
        g = torch.Generator().manual_seed(seed)
        r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(device)
        self.cfg = ops.BlockConfig(C, [3 * C] + [C] * n_mlp, True, True)
        self.x, self.d_out = r(self.V, C), r(self.V, C)
        self.time = (0.01 + 0.3 * torch.rand(C, generator=g)).to(device)
        self.A_re, self.A_im = r(C, C, scale=C ** -0.5), r(C, C, scale=C ** -0.5)
        self.Ws = [r(C, 3 * C, scale=(3 * C) ** -0.5)] + [r(C, C, scale=C ** -0.5) for _ in range(n_mlp - 1)]
        self.bs = [r(C, scale=0.1) for _ in range(n_mlp)]
        self.masks_u8 = [None] + [(torch.rand(self.V, C, generator=g) < 0.5).to(torch.uint8).to(device) for _ in range(n_mlp - 1)]

    def masks(self, dropout):
        return {"none": None, "seeded": 0x1234567, "masks": self.masks_u8}[dropout]

    def fwd(self, dropout, flags=0):
        self.cfg.flags = flags
        try:
            out, saved, _ = ops.block_fwd(self.mb, self.cfg, self.masks(dropout), self.x, self.time, self.A_re, self.A_im, self.Ws, self.bs, None, save=True)
        finally:
            self.cfg.flags = 0
        return out, saved

    def bwd(self, dropout, saved):
        """-> ([d_x, d_time, dA_re, dA_im, dW_0, db_0, ...] on the host, launches and algorithmic bytes of chain_bwd_kernel in this call)"""
        grads = [torch.empty_like(t) for t in (self.time, self.A_re, self.A_im)]
        for w, b in zip(self.Ws, self.bs):
            grads += [torch.empty_like(w), torch.empty_like(b)]
        L = _hip.lib()
        L.dn_prof_reset()
        L.dn_prof_enable(1)
        try:
            d_x, _ = ops.block_bwd(self.mb, self.cfg, self.masks(dropout), self.d_out, self.x, self.time, self.A_re, self.A_im, self.Ws, self.bs, saved, grads)
            rec = (ctypes.c_double * 4)()
            L.dn_prof_read(K_CHAIN_BWD, rec)
        finally:
            L.dn_prof_enable(0)
        return [t.cpu() for t in [d_x] + grads], (int(rec[1]), float(rec[3]))

    def chain_bwd_bytes(self, with_bits):
        """dn_launch_chain_bwd's algorithmic traffic (gradient features on): which of the two forms of the kernel a call launched"""
        VC, n = 4.0 * self.V * self.C, self.n_mlp
        reads = 1 + 5 + (0 if with_bits else n - 1)
        return VC * (reads + (n - 1) + 2 + 3) + (16.0 * self.V * (n - 1) if with_bits else 0.0)


def unpack(words, C):
    """[V, 4] int32 words -> [V, C] bool: bit 4 nt + e of word (row, q) is column 16 nt + 4 q + e"""
    w = words.cpu().to(torch.int64) & 0xFFFFFFFF
    col = torch.arange(C)
    nt, q, e = col // 16, (col % 16) // 4, col % 4
    return ((w[:, q] >> (4 * nt + e)) & 1).bool()


def check_bits(blk, saved):
    hb = saved.hbits
    assert hb.dtype == torch.int32 and tuple(hb.shape) == (blk.n_mlp - 1, blk.V, 4)
    for j, h in enumerate(saved.hs):
        want, got = h.cpu() > 0, unpack(hb[j], blk.C)
        assert torch.equal(got, want), ("layer %d: %d of %d sign bits differ from h > 0" % (j, int((got != want).sum()), want.numel()))
        assert 0 < int(want.sum()) < want.numel()      # (a set of activations with both signs: the comparison says something)
        if blk.C == 64:
            assert int(((hb[j].cpu().to(torch.int64) & 0xFFFFFFFF) >> 16).max()) == 0, "C = 64 uses the low 16 bits"


def run_bits_match_h(device, sizes, C, n_mlp, form, nw, hh, dropouts=("seeded", "masks", "none"), ran_check=True):
    """case 1: after a training forward the unpacked words equal h > 0 for every live row and layer"""
    blk = Block(device, sizes, C, n_mlp, K=128 if form == "spectral" else 32)
    if form == "spectral":
        assert blk.mb.sg_pack is not None, "the batch carries no spectral-gradient operands"
    # (the spectral form exists with one half per wave only; 0 = the gather form whatever the batch carries)
    with options(chain_nw=nw, chain_hh=hh, spectral_grad=2 if form == "spectral" else 0):
        outs = {}
        for dropout in dropouts:
            out, saved = blk.fwd(dropout)
            check_bits(blk, saved)
            outs[dropout] = out.cpu()
        if form == "spectral" and ran_check:
            with options(spectral_grad=0):
                assert not torch.equal(blk.fwd(dropouts[0])[0].cpu(), outs[dropouts[0]]), "spectral and gather form bitwise equal: the spectral form did not run"
    return blk


def run_bwd_bits_vs_h(device, sizes, C, n_mlp, hh, dropout="seeded", fallback=True):
    """cases 2 and 3: the chained backward from the words equals the chained backward from h, bit for bit, on the saved set of the chained
    forward and on the saved set of the unfused forward (DN_BLOCK_NO_CHAIN), whose words come from the pack kernel.  That the words were what
    the kernel read: the same call with every h overwritten by -1 (the weight-gradient products dW_j, j >= 1, read h as values and are left
    out) still gives the same gradients -- from h, every gradient but the biases' would be zero.  On the device the profiling counters name
    the kernel and, through its accounted traffic, the form."""
    blk = Block(device, sizes, C, n_mlp, K=32)
    names = ["d_x", "d_time", "dA_re", "dA_im"] + ["%s_%d" % (k, i) for i in range(n_mlp) for k in ("dW", "db")]
    counted = str(device) != "cpu"      # (the emulator build has no profiling counters)
    with options(chain_hh=hh, spectral_grad=0):
        out_c, saved_c = blk.fwd(dropout)
        sets = [("chained forward", saved_c)]
        if fallback:
            out_u, saved_u = blk.fwd(dropout, flags=NO_CHAIN)
            assert not torch.equal(out_u.cpu(), out_c.cpu()), "chained and unfused forward bitwise equal: the flag changed nothing"
            check_bits(blk, saved_u)
            sets.append(("unfused forward + pack kernel", saved_u))
        for what, saved in sets:
            with_bits, (n1, b1) = blk.bwd(dropout, saved)
            without, (n0, b0) = blk.bwd(dropout, saved._replace(hbits=None))
            if counted:
                assert (n1, b1) == (1, blk.chain_bwd_bytes(True)) and (n0, b0) == (1, blk.chain_bwd_bytes(False)), (what, n1, b1, n0, b0)
            for name, a, b in zip(names, with_bits, without):
                assert torch.equal(a, b), (what, name, "backward from the sign-bit words differs from the backward from h")
            assert float(with_bits[0].abs().max()) > 0
            blind, _ = blk.bwd(dropout, saved._replace(hs=[torch.full_like(h, -1.0) for h in saved.hs]))
            for name, a, b in zip(names, with_bits, blind):
                if not (name.startswith("dW_") and name != "dW_0"):
                    assert torch.equal(a, b), (what, name, "the chained backward read h although the sign-bit words were given")


def run_unchained_backward(device, sizes, C, n_mlp, K):
    """case 4: shapes whose forward is chained and whose backward is not (C = 256; n_mlp = 4): as before, with the words given or not"""
    blk = Block(device, sizes, C, n_mlp, K=K)
    with options(spectral_grad=0):
        out, saved = blk.fwd("seeded")
        out_u, _ = blk.fwd("seeded", flags=NO_CHAIN)
        assert not torch.equal(out.cpu(), out_u.cpu()), "the forward did not take the chained kernel"
        if C <= 128:
            check_bits(blk, saved)
        given, (n1, _) = blk.bwd("seeded", saved)
        null, (n0, _) = blk.bwd("seeded", saved._replace(hbits=None))
        assert n1 == 0 and n0 == 0, "the backward took the chained kernel"
        for a, b in zip(given, null):
            assert torch.equal(a, b)
        assert float(given[0].abs().max()) > 0
