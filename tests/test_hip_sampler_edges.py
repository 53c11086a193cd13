"""GPU: every (marcher, contraction) pair of csrc/sampler.hip and the occupancy-grid kernels against the CPU oracle, bit for bit, at
the sampler's chunk, workgroup and argument edges.  Fixtures: tests/_sampler_cases.py (their conditions are asserted on the oracle
alone in tests/test_sampler_cases.py).  Floats are compared on their bits; every output buffer is pre-filled (NaN, -1, all-ones) so an
element the kernel does not write shows.

Which launch and which branch each case reaches:
A. test_pair_vs_oracle[marcher-contraction-box-S]: all six instantiations of sample_mask_kernel / sample_pack_kernel (with_pair:
   marcher 0..1 x contraction 0..2), on the non-cubic (12, 20, 16) grid, with box ``mixed`` (pow2 == 0: ``/ (hi - lo)``; one axis of it IS a power of two)
   and box ``pow2`` (``* inv_ext``).  S = 1 (one lane of one chunk), 63, 64 (a full chunk), 65 (a second chunk of one lane), 200 (four
   chunks, the last partial).  Three modes: training=False (``a.jitter == nullptr && !a.use_rng``; for (aabb, aabb) the exit shortcut is
   on), an explicit jitter table (shortcut off), the device RNG (``a.use_rng``, shortcut on: the production path; counters r * S + k) --
   each with the coarse early reject (``surely_empty``) on and off.  Through RayProvider: ``info``, ``packed``, ``ray_ids``, ``t``; through
   the ABI: every word of ``maskbits`` (bits at k >= S are zero) and ``counts``.
   test_short_ray_prefixes: R = 1, 3, 4, 5 at S = 65 -- the last workgroup of four waves holds 1, 3, 4 (full) and 1 rays
   (``ray >= n_rays`` return), one pair of each marcher.
B. test_zero_fill_beyond_64_chunks: S = 8256 = 129 chunks, (aabb, aabb), training=False: rays that leave the box early have
   n_active + 64 < n_chunks, so the strided zero-fill loop behind the chunk loop runs (the statement before it covers 64 chunks only).
C. test_pack_arguments: sample_pack_kernel with ``capacity`` below the total (``row < capacity``), a non-null ``base_offset`` in scan
   and pack, and ``ray_ids`` / ``steps`` / ``t_values`` NULL in turn.
D. test_contract_abi: contract_kernel<AABB / MIP360_INF / MIP360_L2> at n = 1, 255, 256, 257 (one 256-thread workgroup, its last
   thread idle / busy, a second workgroup), on the faces of both boxes and their float32 neighbours (the mask is inclusive) and at
   norm 1, its neighbour above, 0, 1e30 and 3e38.  test_march_rays_abi: march_rays_kernel<AABB> with far = 3 (rays that miss clamp to it).
   test_nan_rows_keep_nothing: see below.
E. occupancy_query_kernel on grids with a dimension of 1 or 2 (``W - 1 == 0``: every in-range point reads tap 0 with weight 1) and on
   infinite / NaN points; occupancy_slice_coords_kernel in table and RNG form on a non-cubic grid (the reference's unflipped ``size``),
   and through OccupancyGrid.update's slab batching with a partial last slab; occupancy_apply_kernel; occupancy_stats_kernel with a
   second round of its grid-stride loop (n > 2048 * 256 * 16); occupancy_coarsen_kernel against its definition.

NaN rows (part D).  The kernel's inf-norm is ``fmaxf(fmaxf(|x|, |y|), |z|)``, and fmaxf drops a NaN operand where ``torch.norm`` propagates
it: for a point with ONE NaN component the reference contracts to (NaN, NaN, NaN), tn_contract to NaN in that component only.  The
sampler's mask does not differ -- a NaN coordinate fails every in-bounds test of the trilinear lookup (value 0, not above a threshold
>= 0), and the box contraction's in-box test is false -- so rows with a NaN input are held to one thing only: through tn_sample_mask
none of their candidates is kept.  This is a known, deliberate divergence of tn_contract's output; it is not "fixed".

Findings.  The kernels: none -- every comparison, the Mip-360 L2 pairs included, is bit-equal on an MI355X.  One input of theirs is not
the CPU's: ``RayMarcherAABB.step_size`` is the reference's torch expression ``norm(hi - lo) / n_samples`` evaluated on the device, where
torch divides a tensor by a Python scalar as a multiplication by the rounded reciprocal; at S = 63 that is 1 ulp above the CPU's
division (0x3D94F858 against 0x3D94F857 for box ``pow2``; S = 1, 64, 65, 200 and 8256 agree).  It is torch's own arithmetic on either
side, like ``torch.linspace`` in the unbounded table, and is handled the same way: ``box_marcher`` installs the CPU value in the marcher, so
that the kernels are compared on identical inputs.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import _sampler_cases as sc
from oracle import tinynerf_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


def cu(a, dtype=None):
    t = torch.as_tensor(np.array(a))                                  # (a copy: the fixtures are read-only)
    return (t if dtype is None else t.to(dtype)).to(DEV)


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, f32).view(np.int32)


def same_bits_or_nan(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, f32)
    b = np.asarray(b, f32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


def core():
    from tinynerf_amd import core as c
    return c


def lib():
    from tinynerf_amd import _lib as L
    return L


def dev():
    return torch.device(DEV, torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def dev_rays():
    o, d, _ = sc.rays()
    return cu(o), cu(d)


def box_marcher(box, S, far=1e5):
    m = core().RayMarcherAABB(cu(sc.BOXES[box]), S, sc.NEAR, far)
    host = torch.from_numpy(sc.BOXES[box].copy())
    step = torch.norm(host[1] - host[0]) / S                          # core.py:68-70 by torch's CPU kernels, as the oracle restates it
    assert np.array_equal(bits(step), bits(orc.aabb_step_size(sc.BOXES[box], S)))
    m.__dict__["step_size"] = step                                    # (the cached property; see "Findings" in the module docstring)
    return m


def provider(marcher, contraction, box, S, far=1e5):
    c = core()
    g = sc.grid()
    og = c.OccupancyGrid(list(g.shape), 1 / 1024.).to(DEV)
    og.grid.copy_(cu(g))
    og.mean = sc.THRESHOLD
    assert og.threshold == sc.THRESHOLD
    aabb = cu(sc.BOXES[box])
    if marcher == "aabb":
        m = box_marcher(box, S, far)
    else:
        m = c.RayMarcherUnbounded(S, sc.NEAR, 1e5, sc.UNIFORM_RANGE)
        t, dl = orc.unbounded_table(S, sc.NEAR, sc.UNIFORM_RANGE)
        m._tables[str(dev())] = (cu(t), cu(dl))                       # CPU-linspace table for bit parity
    con = c.ContractionAABB(aabb) if contraction == "aabb" else c.ContractionMip360(sc.ORDER[contraction])
    return c.RayProvider(og, con, m)


def seed_of(key):
    """the seed RayProvider._desc draws after torch.manual_seed(key)"""
    torch.manual_seed(key)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


@functools.lru_cache(maxsize=None)
def reference(marcher, contraction, box, S, mode, n_rays=sc.R):
    """(packed, info, mask, t) of the oracle, computed once per case and shared; read-only"""
    jit = None
    if mode == "table":
        jit = sc.jitter_table(S)[:n_rays]
    elif mode == "rng":
        jit = orc.sampler_jitter(seed_of(4242 + S), n_rays, S)
    out = sc.oracle_sampler(marcher, contraction, box, S, jit, n_rays)
    for a in out:
        a.setflags(write=False)
    return out


def abi_mask(desc, o, d, S):
    L = lib()
    R = o.size(0)
    maskbits = torch.full((R, (S + 63) // 64), -1, dtype=torch.int64, device=DEV)        # all-ones
    counts = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    L.call("tn_sample_mask", dev(), C.byref(desc), L.ptr(o), L.ptr(d), C.c_int64(R), L.ptr(maskbits), L.ptr(counts))
    return maskbits, counts


def check_case(marcher, contraction, box, S, n_rays=sc.R, coarse_modes=(True, False)):
    prov = provider(marcher, contraction, box, S)
    o, d = (x[:n_rays].contiguous() for x in dev_rays())
    for mode in ("eval", "table", "rng"):
        p_ref, i_ref, m_ref, t_ref = reference(marcher, contraction, box, S, mode, n_rays)
        jit = cu(sc.jitter_table(S)[:n_rays]) if mode == "table" else None
        for coarse in coarse_modes:
            tag = (mode, coarse)
            prov.occupancy_grid.use_coarse = coarse
            seed = seed_of(4242 + S)
            torch.manual_seed(4242 + S)
            packed, info, ids, t = prov(o, d, training=mode != "eval", jitter=jit, return_ray_ids=True, return_t=True)
            assert info.dtype == torch.int32 and np.array_equal(info.cpu().numpy(), i_ref), tag
            assert packed.shape == p_ref.shape and np.array_equal(bits(packed), bits(p_ref)), tag
            assert np.array_equal(ids.cpu().numpy(), np.repeat(np.arange(n_rays), i_ref[:, 1])), tag
            assert np.array_equal(bits(t), bits(t_ref)), tag
            # the ABI itself, on pre-filled buffers
            torch.manual_seed(4242 + S)
            desc = prov._desc(dev(), mode != "eval", jit)
            assert (mode != "rng" or (desc.use_rng == 1 and desc.seed == seed)) and bool(desc.coarse) == coarse
            maskbits, counts = abi_mask(desc, o, d, S)
            words = maskbits.cpu().numpy().view(np.uint64)
            assert np.array_equal(words, sc.pack_mask(m_ref)), tag                        # (bits at k >= S: zero in pack_mask)
            assert np.array_equal(counts.cpu().numpy(), i_ref[:, 1]), tag
    if S >= 63 and n_rays == sc.R:
        assert not np.array_equal(reference(marcher, contraction, box, S, "eval")[2], reference(marcher, contraction, box, S, "rng")[2])


# ---------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("S", sc.S_VALUES)
@pytest.mark.parametrize("box", list(sc.BOXES))
@pytest.mark.parametrize("marcher,contraction", sc.PAIRS)
def test_pair_vs_oracle(marcher, contraction, box, S):
    check_case(marcher, contraction, box, S)


@pytest.mark.parametrize("n_rays", sc.R_PREFIXES)
@pytest.mark.parametrize("marcher,contraction", [("aabb", "aabb"), ("unbounded", "mip360_inf")])
def test_short_ray_prefixes(marcher, contraction, n_rays):
    for box in sc.BOXES:
        check_case(marcher, contraction, box, 65, n_rays)


# ---------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("box", list(sc.BOXES))
def test_zero_fill_beyond_64_chunks(box):
    S, R = sc.S_LONG, sc.R_LONG
    prov = provider("aabb", "aabb", box, S)
    o, d = (x[:R].contiguous() for x in dev_rays())
    p_ref, i_ref, m_ref, _ = reference("aabb", "aabb", box, S, "eval", R)
    ref_words = sc.pack_mask(m_ref)
    assert ref_words.shape == (R, 129)
    last = np.array([np.flatnonzero(w).max() if w.any() else -1 for w in ref_words])
    assert ((last >= 0) & (last + 66 < 129)).any()            # a ray with samples whose last occupied chunk leaves > 64 chunks behind it
    desc = prov._desc(dev(), False, None)
    maskbits, counts = abi_mask(desc, o, d, S)
    assert np.array_equal(maskbits.cpu().numpy().view(np.uint64), ref_words)
    assert np.array_equal(counts.cpu().numpy(), i_ref[:, 1])
    packed, info = prov(o, d, training=False)                                         # exit shortcut on
    p0, i0 = prov(o, d, training=True, jitter=torch.zeros(R, S, device=DEV))          # t + 0 * delta: same candidates, shortcut off
    for p, i in ((packed, info), (p0, i0)):
        assert np.array_equal(i.cpu().numpy(), i_ref) and np.array_equal(bits(p), bits(p_ref))


# ---------------------------------------------------------------------------------------------- C
def _pack(desc, o, d, maskbits, info, base, rows, capacity, skip=None):
    L = lib()
    out = {"packed": torch.full((rows, 7), float("nan"), device=DEV), "ray_ids": torch.full((rows,), -1, dtype=torch.int32, device=DEV),
           "steps": torch.full((rows,), float("nan"), device=DEV), "t": torch.full((rows,), float("nan"), device=DEV)}
    arg = {k: (None if k == skip else v) for k, v in out.items()}
    L.call("tn_sample_pack_t", dev(), C.byref(desc), L.ptr(o), L.ptr(d), C.c_int64(o.size(0)), L.ptr(maskbits), L.ptr(info), L.ptr(base),
           L.ptr(arg["packed"]), L.ptr(arg["ray_ids"]), L.ptr(arg["steps"]), L.ptr(arg["t"]), C.c_int64(capacity))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _filled(name, a):
    return (a == -1).all() if name == "ray_ids" else np.isnan(a).all()


@pytest.mark.parametrize("marcher,contraction", [("aabb", "aabb"), ("unbounded", "mip360_inf")])
def test_pack_arguments(marcher, contraction):
    L = lib()
    S, R, box = 200, sc.R, "mixed"
    prov = provider(marcher, contraction, box, S)
    o, d = dev_rays()
    p_ref, i_ref, m_ref, t_ref = reference(marcher, contraction, box, S, "eval")
    total = int(i_ref[:, 1].sum())
    assert total == p_ref.shape[0] and total > 1000
    desc = prov._desc(dev(), False, None)
    maskbits, counts = abi_mask(desc, o, d, S)
    info = torch.full((R, 2), -1, dtype=torch.int32, device=DEV)
    tot = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    L.call("tn_sample_scan", dev(), L.ptr(counts), C.c_int64(R), C.c_void_p(None), L.ptr(info), L.ptr(tot))
    assert np.array_equal(info.cpu().numpy(), i_ref) and int(tot.item()) == total
    want = {"packed": p_ref, "ray_ids": np.repeat(np.arange(R, dtype=np.int32), i_ref[:, 1]), "steps": p_ref[:, 6], "t": t_ref}

    def equal(name, got, rows=slice(None)):
        return np.array_equal(got[rows], want[name][rows]) if name == "ray_ids" else np.array_equal(bits(got[rows]), bits(want[name][rows]))

    full = _pack(desc, o, d, maskbits, info, None, total, total)
    assert all(equal(k, full[k]) for k in want)
    # capacity below the total: rows below it as in the full pack, rows at and above it untouched in every output
    cap = total // 2
    part = _pack(desc, o, d, maskbits, info, None, total, cap)
    for k in want:
        assert equal(k, part[k], slice(0, cap)) and _filled(k, part[k][cap:]), k
    # a base offset: the scan adds it, the pack takes it off again
    base = torch.tensor([12345], dtype=torch.int32, device=DEV)
    info_b = torch.full((R, 2), -1, dtype=torch.int32, device=DEV)
    L.call("tn_sample_scan", dev(), L.ptr(counts), C.c_int64(R), L.ptr(base), L.ptr(info_b), L.ptr(tot))
    assert np.array_equal(info_b.cpu().numpy(), i_ref + np.array([12345, 0], np.int32)) and int(tot.item()) == total
    shifted = _pack(desc, o, d, maskbits, info_b, base, total, total)
    assert all(equal(k, shifted[k]) for k in want)
    # each optional output NULL in turn: the others unchanged, the skipped buffer untouched
    for skip in ("ray_ids", "steps", "t"):
        got = _pack(desc, o, d, maskbits, info, None, total, total, skip=skip)
        for k in want:
            assert _filled(k, got[k]) if k == skip else equal(k, got[k]), (skip, k)


# ---------------------------------------------------------------------------------------------- D
def _contract(desc, pts):
    L = lib()
    n = pts.shape[0]
    x = cu(pts)
    out = torch.full((n + 1, 3), float("nan"), device=DEV)              # one guard row behind the n the kernel may write
    mask = torch.full((n + 1,), 255, dtype=torch.uint8, device=DEV)
    L.call("tn_contract", dev(), C.byref(desc), L.ptr(x), C.c_int64(n), L.ptr(out), L.ptr(mask))
    out, mask = out.cpu().numpy(), mask.cpu().numpy()
    assert np.isnan(out[n]).all() and mask[n] == 255
    return out[:n], mask[:n]


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_contract_abi(n):
    L = lib()
    c = core()
    for box, aabb in sc.BOXES.items():
        pts = sc.box_points(box)[:n]
        desc = L.SamplerDesc(n_samples=1)
        c.ContractionAABB(cu(aabb))._describe(desc)
        out, mask = _contract(desc, pts)
        ref, ref_mask = orc.contract_aabb(pts, aabb)
        assert same_bits_or_nan(out, ref), box
        assert np.array_equal(mask, ref_mask.astype(np.uint8)), box         # inclusive: on a face is inside, one ulp out is not
    pts = sc.mip_points()[:n]
    for name, order in sc.ORDER.items():
        desc = L.SamplerDesc(n_samples=1)
        c.ContractionMip360(order)._describe(desc)
        out, mask = _contract(desc, pts)
        with np.errstate(all="ignore"):
            ref, _ = orc.contract_mip360(pts, order)
        assert same_bits_or_nan(out, ref), name
        assert (mask == 1).all()


@pytest.mark.parametrize("S", [1, 17])
def test_march_rays_abi(S):
    L = lib()
    o, d = dev_rays()
    o_np, d_np, _ = sc.rays()
    for box, aabb in sc.BOXES.items():
        m = box_marcher(box, S, 3.0)
        desc = L.SamplerDesc()
        m._describe(desc, dev())
        t = torch.full((sc.R, S), float("nan"), device=DEV)
        dl = torch.full((sc.R, S), float("nan"), device=DEV)
        L.call("tn_march_rays", dev(), C.byref(desc), L.ptr(o), L.ptr(d), C.c_int64(sc.R), L.ptr(t), L.ptr(dl))
        t_ref, dl_ref = orc.march_aabb(o_np, d_np, aabb, S, sc.NEAR, 3.0)
        assert np.array_equal(bits(t), bits(t_ref)) and np.array_equal(bits(dl), bits(dl_ref))
        assert (t_ref[:, 0] == 3.0).any() and (t_ref[:, 0] == f32(sc.NEAR)).any() and ((t_ref[:, 0] > sc.NEAR) & (t_ref[:, 0] < 3)).any()


@pytest.mark.parametrize("marcher,contraction", sc.PAIRS)
def test_nan_rows_keep_nothing(marcher, contraction):
    """A NaN in a ray's origin or direction makes every candidate point hold a NaN: none is kept, with and without the coarse reject, and
    the rays next to them are not disturbed.  (What tn_contract itself writes for such a point differs from the reference in the non-NaN
    components -- fmaxf drops a NaN, torch.norm propagates it; see the module docstring -- and is deliberately not compared.)"""
    S, n = 65, 12
    o_np, d_np, _ = sc.rays()
    o_np, d_np = o_np[:n].copy(), d_np[:n].copy()
    for i in range(0, n, 2):
        (o_np if i % 4 == 0 else d_np)[i, (i // 2) % 3] = np.nan
    prov = provider(marcher, contraction, "mixed", S)
    _, _, m_ref, _ = reference(marcher, contraction, "mixed", S, "eval", n)
    want = sc.pack_mask(m_ref)
    want[0::2] = 0
    assert want[1::2].any()
    for coarse in (True, False):
        prov.occupancy_grid.use_coarse = coarse
        desc = prov._desc(dev(), False, None)
        maskbits, counts = abi_mask(desc, cu(o_np), cu(d_np), S)
        assert np.array_equal(maskbits.cpu().numpy().view(np.uint64), want)
        assert (counts.cpu().numpy()[0::2] == 0).all()


# ---------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("shape", sc.TRILINEAR_SHAPES)
def test_occupancy_query_abi(shape):
    L = lib()
    g, p = sc.trilinear_grid(shape), sc.trilinear_points(shape)
    with np.errstate(all="ignore"):
        ref = orc.trilinear_zeros_align(g, p)
    pos = np.sort(ref[ref > 0])
    thr = float(pos[len(pos) // 2])                              # a value the lookup returns: `>` must give 0 there
    D, H, W = shape
    n = p.shape[0]
    gt, pt = cu(g), cu(p)
    for want_out, want_val in ((True, True), (True, False), (False, True)):
        out = torch.full((n,), 2, dtype=torch.uint8, device=DEV)
        vals = torch.full((n,), float("nan"), device=DEV)
        L.call("tn_occupancy_query", dev(), L.ptr(gt), C.c_int(D), C.c_int(H), C.c_int(W), L.ptr(pt), C.c_int64(n), C.c_float(thr),
               L.ptr(out if want_out else None), L.ptr(vals if want_val else None))
        if want_val:
            assert same_bits_or_nan(vals, ref) and not np.isnan(ref).any()
        else:
            assert bool(torch.isnan(vals).all())
        if want_out:
            got = out.cpu().numpy()
            assert np.array_equal(got, (ref > f32(thr)).astype(np.uint8))
            assert (got[ref == f32(thr)] == 0).all() and (ref == f32(thr)).any() and (got.any() or g.size == 1)
        else:
            assert bool((out == 2).all())


def _slice_coords(size, i, jitter, seed):
    L = lib()
    D, H, W = size
    out = torch.full((H * W + 1, 3), float("nan"), device=DEV)
    L.call("tn_occupancy_slice_coords", dev(), C.c_int(D), C.c_int(H), C.c_int(W), C.c_int(i), L.ptr(jitter), C.c_uint64(seed), L.ptr(out))
    out = out.cpu().numpy()
    assert np.isnan(out[H * W]).all()
    return out[:H * W]


def _refresh_uniforms(size, i, seed):
    """the refresh's counters: voxel (slice, j) coordinate c draws (slice * H * W + j) * 3 + c"""
    D, H, W = size
    ctr = ((np.uint64(i) * np.uint64(H * W) + np.arange(H * W, dtype=np.uint64))[:, None] * np.uint64(3) + np.arange(3, dtype=np.uint64)[None])
    return orc.uniform01(seed, ctr).reshape(H, W, 3)


def test_occupancy_slice_coords_and_update_batching():
    size = (5, 12, 20)
    D, H, W = size
    seed = 0x1234_5678_9ABC_DEF
    rng = np.random.default_rng(8)
    ref_rng = []
    for i in range(D):
        jit = rng.random((H, W, 3), dtype=f32)
        assert np.array_equal(bits(_slice_coords(size, i, cu(jit), 0)), bits(orc.occupancy_voxel_coords(size, i, jit)))
        u = _refresh_uniforms(size, i, seed)
        assert u.min() >= 0 and u.max() < 1 and len(np.unique(u)) > 0.99 * u.size
        ref_rng.append(orc.occupancy_voxel_coords(size, i, u))
        assert np.array_equal(bits(_slice_coords(size, i, None, seed)), bits(ref_rng[-1]))
    # OccupancyGrid.update: slabs of 3 and 2 slices, written at coords + j * H * W * 12 bytes, applied to grid[i0 : i0 + n_sl]
    og = core().OccupancyGrid(list(size), 1 / 1024.).to(DEV)
    cells0 = (1.0 - rng.random(size)).astype(f32)
    og.grid.copy_(cu(cells0))
    seen = []

    def sigma_fn(pts):
        seen.append(pts.clone())
        first = sum(s.size(0) for s in seen[:-1])
        idx = torch.arange(first, first + pts.size(0), device=pts.device)
        return torch.where(idx % 3 == 0, 1000.0, 0.0)             # alpha = 1 - exp(-1000 / 1024) or 0: far from the threshold

    og.update(sigma_fn, seed=seed, slices_per_call=3)
    assert [s.size(0) for s in seen] == [3 * H * W, 2 * H * W]
    assert np.array_equal(bits(torch.cat(seen)), bits(np.concatenate(ref_rng)))
    hit = (np.arange(D * H * W) % 3 == 0).reshape(size)
    want = np.where(hit, f32(1), (f32(og.decay) * cells0).astype(f32))
    assert np.array_equal(bits(og.grid), bits(want))
    assert og.mean == pytest.approx(float(want.astype(np.float64).mean()), rel=1e-12)


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_occupancy_apply_abi(n):
    L = lib()
    step, thr, decay = 1 / 1024., 0.01, 0.95
    cells, sig, alpha, redrawn = sc.apply_case(n, step, thr)
    assert redrawn < 0.01 * n or (n == 1 and redrawn == 0)
    buf = torch.full((n + 1,), float("nan"), device=DEV)
    buf[:n] = cu(cells)
    L.call("tn_occupancy_apply", dev(), L.ptr(buf), L.ptr(cu(sig)), C.c_int64(n), C.c_float(step), C.c_float(thr), C.c_float(decay))
    with np.errstate(invalid="ignore"):
        want = np.where(alpha > np.float64(f32(thr)), f32(1), (f32(decay) * cells).astype(f32))       # a NaN alpha decays the cell
    got = buf.cpu().numpy()
    assert np.isnan(got[n]) and np.array_equal(bits(got[:n]), bits(want))
    assert (want[np.isnan(sig)] == (f32(decay) * cells[np.isnan(sig)]).astype(f32)).all() and np.isnan(sig).any()


@pytest.mark.parametrize("n", [0, 1, 255, 4097, 2048 * 256 * 16 + 4099])
def test_occupancy_stats_abi(n):
    """count exact; |sum - fsum| <= 2 n 2^-53 sum |v|: twice the bound of ANY order of n float64 additions of the (exactly converted)
    float32 cells, (n - 1) u sum |v| to first order -- derived, not measured.  The last size gives the first 4099 threads of the
    2048 x 256 grid a 17th element, one stride behind their 16th: the second round of the grid-stride loop."""
    L = lib()
    rng = np.random.default_rng(n + 1)
    v = rng.random(max(n, 1), dtype=f32)
    v[rng.random(v.size) < 0.3] = f32(0.01)                       # the threshold itself, many times: `>` must not count it
    v[rng.random(v.size) < 0.05] = 0.0
    stats = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    L.call("tn_occupancy_stats", dev(), L.ptr(cu(v)), C.c_int64(n), C.c_float(0.01), L.ptr(stats))
    s, c = stats.tolist()
    v = v[:n]
    assert c == float((v > f32(0.01)).sum())
    exact = math.fsum(v.astype(np.float64).tolist())
    assert abs(s - exact) <= 2 * n * 2.0 ** -53 * exact, (s, exact)          # (v >= 0: sum |v| = sum v)
    assert n < 255 or (v == f32(0.01)).sum() > 0.2 * n


@pytest.mark.parametrize("shape", sc.COARSEN_SHAPES)
def test_occupancy_coarsen_abi(shape):
    """Block b of an axis covers cells 4b .. min(4b + 4, N - 1), the maximum clamped at 0.  That halo covers every tap: a point whose
    floor index x0 falls in block b (4b <= max(x0, 0) <= 4b + 3, ``surely_empty``) reads taps x0 and x0 + 1 <= 4b + 4 only, and a tap
    outside the grid contributes 0, which the clamp accounts for."""
    L = lib()
    g = sc.coarsen_grid(shape)
    ref = sc.coarsen_ref(g)
    D, H, W = shape
    out = torch.full((ref.size + 1,), float("nan"), device=DEV)
    L.call("tn_occupancy_coarsen", dev(), L.ptr(cu(g)), C.c_int(D), C.c_int(H), C.c_int(W), L.ptr(out))
    out = out.cpu().numpy()
    assert np.isnan(out[ref.size]) and np.array_equal(bits(out[:ref.size]), bits(ref.reshape(-1)))
    # ... and OccupancyGrid.coarse_maxima hands the sampler the same table
    og = core().OccupancyGrid(list(shape), 1 / 1024.).to(DEV)
    og.grid.copy_(cu(g))
    assert np.array_equal(bits(og.coarse_maxima()), bits(ref))
