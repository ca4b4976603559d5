"""GPU tests of the candidate refinement (refine_kernels.hip through rt_refine
and rt_refine_device): profiles bit for bit against the host specification at
every kernel path (every bins-per-thread group, one to three chunks of shift
rows in either stage, every count of widths per wave), batching, device tables
that were never validated, S/N of profiles with a large offset, recovery of an
off-centre trial, and a candidate refined straight from a file."""
import ctypes

import numpy as np
import pytest

import dedisp_common as dc
import refine_common as rc
from conftest import snr_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# (B, S, N, K, J): the smallest, odd sizes, around one wave and one block of
# bins, the widest profile, and the two sides of the 64 KiB LDS stage of stage
# B (S * N * 4 = 65536 and 67584); (32, 4, 255) and (5, 3, 257) take two bins
# per thread or an idle tail
SHAPES = [(1, 1, 2, 1, 1), (2, 1, 3, 3, 2), (7, 2, 63, 3, 3), (7, 2, 64, 3, 3), (7, 2, 65, 3, 3), (32, 4, 255, 2, 3),
          (5, 3, 257, 2, 2), (2, 2, 1024, 2, 2), (2, 32, 512, 3, 3), (2, 33, 512, 3, 3)]
# A thread owns E = ceil(N / 256) bins, one instantiation of the trial loop per
# E: 256 is E = 1 with no idle lane; 513 (one live lane in the last group), 700
# and 768 (none idle) are E = 3; 769 (one live lane) and 1023 (one idle) E = 4
BIN_GROUP_SHAPES = [(3, 2, N, 2, 2) for N in (256, 513, 700, 768, 769, 1023)]
# The shifts of a trial are loaded 256 rows at a time into one of two buffers
# that alternate from chunk to chunk, through every trial of the block.  Rows
# of stage A are bands: one chunk that is also the largest staged slice (64
# KiB), two chunks, three chunks staged (63612 bytes), three chunks read from
# global memory.  Rows of stage B are sub-integrations: the same four.
CHUNK_SHAPES = [(256, 2, 64, 2, 2), (257, 2, 16, 2, 2), (513, 1, 31, 2, 2), (513, 2, 64, 2, 2),
                (2, 256, 64, 2, 2), (2, 257, 16, 2, 3), (2, 513, 31, 2, 2), (2, 513, 64, 2, 2)]
# three chunks a trial: the buffer a trial starts in alternates, and five
# trials start in each of the two more than once
PARITY_SHAPES = [(513, 2, 16, 5, 2), (2, 513, 16, 2, 5)]

job = rc.job


@pytest.mark.parametrize("B,S,N,K,J", SHAPES + BIN_GROUP_SHAPES + CHUNK_SHAPES + PARITY_SHAPES)
def test_bit_identity(torch, B, S, N, K, J):
    from riptide_amd.refine import refine_host, refine_many
    g = job(B, S, N, K, J, "normal")
    assert B * S * 8 < 2 ** 24                               # the integer cube's sums are exact
    for t, rows in ((g[1], B), (g[2], S)):
        # more than one chunk of shifts: chunks that differ, N - 1 | 0 across the chunk boundary
        assert t.shape[1] == rows
        if rows > rc.CHUNK:
            rc.check_chunked_table(t, N)
    if B > 1:
        assert g[1].max() == N - 1 and g[1].min() == 0       # 0 and N - 1 together
    if S > 1:
        assert g[2].max() == N - 1 and g[2].min() == 0
    assert g[3][0] == 1 and g[3][-1] == N - 1
    snr, prof = refine_many([g], profiles=True)[0]
    hsnr, hprof = refine_host(*g, profiles=True)
    assert prof.shape == (K, J, N) and np.array_equal(bits(prof), bits(hprof))
    ok, msg = snr_close(snr, hsnr, rtol=1e-4)
    assert ok, msg
    # small integers: exact against numpy
    g = job(B, S, N, K, J, "int")
    snr, prof = refine_many([g], profiles=True)[0]
    ref, _ = rc.numpy_profiles(g[0], g[1], g[2])
    assert np.array_equal(prof.astype(np.float64), ref)
    ok, msg = snr_close(snr, refine_host(*g), rtol=1e-4)
    assert ok, msg


def test_stage_a_global_path(torch):
    """A slice of stage A past the LDS stage (bands * bins * 4 > 64 KiB): the
    rows are read from global memory, the same bits."""
    from riptide_amd.refine import refine_host, refine_many
    g = job(33, 2, 512, 2, 2, "normal")
    snr, prof = refine_many([g], profiles=True)[0]
    hsnr, hprof = refine_host(*g, profiles=True)
    assert np.array_equal(bits(prof), bits(hprof))
    ok, msg = snr_close(snr, hsnr, rtol=1e-4)
    assert ok, msg


def test_batching(torch):
    """Five candidates of different shapes in one call equal each alone, bit
    for bit; without the profile output the S/N is unchanged."""
    from riptide_amd.refine import refine_many
    jobs = [job(*s, "normal", seed=7) for s in [(3, 2, 64, 2, 3), (1, 1, 2, 1, 1), (2, 33, 512, 2, 2), (7, 5, 257, 3, 1),
                                                (4, 4, 100, 1, 4)]]
    together = refine_many(jobs, profiles=True)
    for g, (snr, prof) in zip(jobs, together):
        s1, p1 = refine_many([g], profiles=True)[0]
        assert np.array_equal(bits(snr), bits(s1)) and np.array_equal(bits(prof), bits(p1))
    for (snr, _), alone in zip(together, refine_many(jobs)):
        assert np.array_equal(bits(snr), bits(alone))


@pytest.mark.parametrize("B,S,N,K,J", [(7, 2, 65, 2, 2), (3, 2, 700, 2, 2)])
def test_width_counts(torch, oracle, B, S, N, K, J):
    """A wave takes the widths w, w + 4, ...: one to three of them with lists
    of 1, 4, 5, 8 and 9 widths, sixteen with 64 (every width of 65 bins), and
    a list that is neither sorted nor free of repeats (the host checks the
    range alone).  The S/N of a width does not depend on its place in a list
    or on the list's length: it has the bits of that width passed alone."""
    from riptide_amd.refine import refine_host, refine_many
    x, d, p, _, stdnoise = job(B, S, N, K, J, "normal", seed=5)
    every = np.arange(1, N) if N <= 65 else np.unique(np.linspace(1, N - 1, 64).astype(np.int64))
    spread = np.unique(np.linspace(1, N - 1, 9).astype(np.int64))
    assert every.size == 64 and spread.size == 9
    lists = [spread[:c] for c in (1, 4, 5, 8, 9)] + [every, np.array([N - 1, 3, 1, N // 2, 3, 2, N - 1, 3, 7, 1, 5])]
    jobs = [(x, d, p, w.astype(np.uint32), stdnoise) for w in lists]
    got = refine_many(jobs, profiles=True)
    _, hprof = refine_host(*jobs[0], profiles=True)
    # every distinct width alone: a batch of one-width candidates
    distinct = np.unique(np.concatenate(lists))
    alone = dict(zip(distinct, refine_many([(x, d, p, [w], stdnoise) for w in distinct])))
    for w, (snr, prof) in zip(lists, got):
        assert snr.shape == (K, J, w.size) and np.array_equal(bits(prof), bits(hprof))
        ok, msg = snr_close(snr, refine_host(x, d, p, w, stdnoise), rtol=1e-4)
        assert ok, (w.size, msg)
        ok, msg = snr_close(snr.reshape(-1, w.size), oracle.snr2(prof.reshape(-1, N), w, stdnoise), rtol=1e-4)
        assert ok, (w.size, msg)
        for i, wi in enumerate(w):
            assert np.array_equal(bits(snr[:, :, i]), bits(alone[wi][:, :, 0])), (w.size, i, wi)


def _device_call(torch, cubes, shifts, widths, table, nsnr, nprof):
    """rt_refine_device on the current stream with outputs of nsnr and nprof
    floats that hold NaN wherever the call writes nothing: (snr, prof) as
    numpy arrays."""
    from riptide_amd import _lib
    L = _lib.load()
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (cubes, shifts, widths.astype(np.int32))]
    snr = torch.full((nsnr,), float("nan"), dtype=torch.float32, device="cuda")
    prof = torch.full((nprof,), float("nan"), dtype=torch.float32, device="cuda")
    need = ctypes.c_size_t()
    _lib.check(L.rt_refine_workspace_bytes(_lib.ptr(table), table.size, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    _lib.check(L.rt_refine_device(_lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(table), table.size,
                                  _lib.ptr(snr), _lib.ptr(prof), _lib.ptr(ws), ws.numel(),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return snr.cpu().numpy(), prof.cpu().numpy()


def test_device_width_clamp(torch):
    """engine.refine_device clamps a width to [1, bins - 1]: 0, N, N + 5 and
    2^31 - 1 give the S/N of 1, N - 1, N - 1 and N - 1, the columns of the
    legal widths beside them are unchanged, and nothing is written outside a
    candidate's [snr_off, snr_off + K J W)."""
    from riptide_amd import engine
    from riptide_amd.refine import pack_refine, refine_many
    shapes = [(5, 4, 100, 3, 3), (3, 2, 65, 2, 2)]
    base = [job(*s, "normal", seed=9) for s in shapes]
    given, legal = [], []
    for g, (_, _, N, _, _) in zip(base, shapes):
        given.append(g[:3] + (np.array([1, 0, N // 3, N, N - 1, N + 5, 2 ** 31 - 1, 2], dtype=np.uint32), g[4]))
        legal.append(g[:3] + (np.array([1, 1, N // 3, N - 1, N - 1, N - 1, N - 1, 2], dtype=np.uint32), g[4]))
    cubes, shifts, widths, table, _, nsnr, nprof = pack_refine(given)
    lwidths = pack_refine(legal)[2]
    assert widths.astype(np.int32).max() == 2 ** 31 - 1 and not np.array_equal(widths, lwidths)
    # guards before, between and after the two candidates' S/N
    table["snr_off"] += 7
    table["snr_off"][1] += 11
    nsnr += 7 + 11 + 5
    snr, prof = _device_call(torch, cubes, shifts, widths, table, nsnr, nprof)
    lsnr, lprof = _device_call(torch, cubes, shifts, lwidths, table, nsnr, nprof)
    assert np.array_equal(bits(snr), bits(lsnr)) and np.array_equal(bits(prof), bits(lprof))
    used = np.zeros(nsnr, dtype=bool)
    for i, (want, (_, _, N, K, J)) in enumerate(zip(refine_many(legal), shapes)):
        o = int(table["snr_off"][i])
        assert not used[o:o + want.size].any()
        used[o:o + want.size] = True
        assert np.array_equal(bits(snr[o:o + want.size]), bits(want.ravel())), i
    assert used.sum() == nsnr - 23 and np.isnan(snr[~used]).all() and not np.isnan(snr[used]).any()
    # the documented entry point itself
    dev = "cuda"
    esnr, _ = engine.refine_device(torch.from_numpy(cubes).to(dev), torch.from_numpy(shifts).to(dev),
                                   torch.from_numpy(widths.astype(np.int32)).to(dev), table)
    torch.cuda.synchronize()
    esnr = esnr.cpu().numpy()
    assert esnr.size == nsnr - 5 and np.array_equal(bits(esnr[used[:-5]]), bits(snr[used]))


@pytest.fixture(scope="module")
def batch40(torch):
    """(jobs, (snr, prof) of each candidate run alone)."""
    from riptide_amd.refine import refine_many
    jobs = rc.batch_jobs()
    assert len(jobs) == 40 and max(g[0].size for g in jobs) <= 8 * 8 * 100
    return jobs, [refine_many([g], profiles=True)[0] for g in jobs]


def test_batch_of_forty(torch, batch40):
    """Forty candidates in one call: each one's S/N and profiles have the bits
    of that candidate run alone.  The kernels find a block's candidate by a
    binary search of the table, here six steps deep, with a candidate of one
    block in both stages first, in the middle and last."""
    from riptide_amd.refine import refine_many
    jobs, alone = batch40
    shapes = rc.batch_shapes()
    assert len(set(shapes)) == 9 and all(1 <= K <= 4 and 1 <= J <= 4 for _, _, _, K, J in shapes)
    for i in (0, 20, 39):
        assert shapes[i][1] == 1 and shapes[i][3] == 1
    assert any(s[1] == 1 and s[3] > 1 for s in shapes) and any(s[3] == 1 and s[1] > 1 for s in shapes)
    together = refine_many(jobs, profiles=True)
    for i, ((snr, prof), (s1, p1)) in enumerate(zip(together, alone)):
        assert np.array_equal(bits(snr), bits(s1)) and np.array_equal(bits(prof), bits(p1)), (i, shapes[i])
    for i, (snr, (s1, _)) in enumerate(zip(refine_many(jobs), alone)):
        assert np.array_equal(bits(snr), bits(s1)), (i, shapes[i])


NAN_BITS = 0x7FC00000       # a float32 NaN; as a shift or a width, a value far from any legal one


def _scattered(jobs, seed):
    """The arrays of one rt_refine_device call for `jobs` with the table in
    reverse order and each candidate's cube, two shift tables, widths, S/N and
    profiles at places unrelated to table order (a permutation of their own
    per array), 1 to 8 unused elements before, between and after them: NaN in
    the cubes, NAN_BITS in the integer arrays.  (cubes, shifts, widths, table,
    S/N floats, profile floats)."""
    from riptide_amd.refine import REFINE_SPEC, _as_job
    rng = np.random.RandomState(seed)
    parts = [_as_job(*g) for g in jobs[::-1]]
    n = len(parts)
    table = np.zeros(n, dtype=REFINE_SPEC)

    def place(sizes):
        off, offs = int(rng.randint(1, 9)), np.zeros(len(sizes), dtype=np.int64)
        for k in rng.permutation(len(sizes)):
            offs[k] = off
            off += sizes[k] + int(rng.randint(1, 9))
        assert not np.array_equal(np.argsort(offs), np.arange(len(sizes)))
        return offs, off

    co, nc = place([x.size for x, _, _, _, _ in parts])
    so, ns = place([d.size for _, d, _, _, _ in parts] + [p.size for _, _, p, _, _ in parts])
    wo, nw = place([w.size for _, _, _, w, _ in parts])
    zo, nsnr = place([d.shape[0] * p.shape[0] * w.size for _, d, p, w, _ in parts])
    po, nprof = place([d.shape[0] * p.shape[0] * x.shape[2] for x, d, p, _, _ in parts])
    cubes = np.full(nc, np.nan, dtype=np.float32)
    shifts = np.full(ns, NAN_BITS, dtype=np.int32)
    widths = np.full(nw, NAN_BITS, dtype=np.uint32)
    for i, (x, d, p, w, stdnoise) in enumerate(parts):
        B, S, N = x.shape
        table[i] = (co[i], so[i], so[n + i], wo[i], zo[i], po[i], B, S, N, d.shape[0], p.shape[0], w.size, stdnoise, 0)
        cubes[co[i]:co[i] + x.size] = x.ravel()
        shifts[so[i]:so[i] + d.size] = d.ravel()
        shifts[so[n + i]:so[n + i] + p.size] = p.ravel()
        widths[wo[i]:wo[i] + w.size] = w
    return cubes, shifts, widths, table, nsnr, nprof


def _check_scattered(table, snr, prof, want, gaps):
    """Candidate i of `table` is want[-1 - i]; with gaps=True everything else
    of snr and prof is still NaN."""
    used_s, used_p = np.zeros(snr.size, dtype=bool), np.zeros(prof.size, dtype=bool)
    for i, (s1, p1) in enumerate(want[::-1]):
        o, q = int(table["snr_off"][i]), int(table["prof_off"][i])
        assert np.array_equal(bits(snr[o:o + s1.size]), bits(s1.ravel())), i
        assert np.array_equal(bits(prof[q:q + p1.size]), bits(p1.ravel())), i
        used_s[o:o + s1.size] = True
        used_p[q:q + p1.size] = True
    if gaps:
        assert not used_s.all() and np.isnan(snr[~used_s]).all() and np.isnan(prof[~used_p]).all()


def test_batch_reversed_with_permuted_offsets(torch, batch40):
    """The forty through rt_refine_device with the table reversed and every
    array of every candidate somewhere else, NaN between them: the same bits.
    Nothing outside a candidate's own ranges is read (a NaN would show in the
    sums, NAN_BITS as a shift or a width would change them) or written.  Once
    more through engine.refine_device on a stream of its own."""
    from riptide_amd import engine
    jobs, alone = batch40
    cubes, shifts, widths, table, nsnr, nprof = _scattered(jobs, seed=1)
    assert np.isnan(cubes).sum() >= 41 and (shifts == NAN_BITS).sum() >= 81
    assert table["bins"][0] == jobs[-1][0].shape[2] and table["cube_off"][0] != 0
    snr, prof = _device_call(torch, cubes, shifts, widths, table, nsnr, nprof)
    _check_scattered(table, snr, prof, alone, gaps=True)
    cubes, shifts, widths, table, nsnr, nprof = _scattered(jobs, seed=2)
    dev = [torch.from_numpy(a).cuda() for a in (cubes, shifts, widths.astype(np.int32))]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    snr, prof = engine.refine_device(*dev, table, profiles=True, stream=side)
    side.synchronize()
    _check_scattered(table, snr.cpu().numpy(), prof.cpu().numpy(), alone, gaps=False)


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0), (1, 0, 2)])
def test_batch_of_staged_and_unstaged(torch, order):
    """A slice staged in LDS and one read from global memory in the same
    launch, in each stage and in every order: a launch's dynamic LDS is the
    largest staged slice's, whichever candidate comes first."""
    from riptide_amd.refine import refine_many
    shapes = [(2, 2, 64, 2, 2), (513, 2, 64, 2, 2), (2, 513, 64, 2, 2)]
    jobs = [job(*shapes[i], "normal", seed=13) for i in order]
    together = refine_many(jobs, profiles=True)
    for g, (snr, prof) in zip(jobs, together):
        s1, p1 = refine_many([g], profiles=True)[0]
        assert np.array_equal(bits(snr), bits(s1)) and np.array_equal(bits(prof), bits(p1)), g[0].shape


@pytest.mark.parametrize("B,S,N,K,J", rc.OFFSET_SHAPES)
def test_snr_with_an_offset(torch, B, S, N, K, J):
    """Profiles about 100 B S high (sub-band folds need not be mean-free when
    stdnoise is given): the same profile bits, and an S/N within the rounding
    of the two large terms of (h + b) * dmax - b * sum of the host's value
    (rc.snr1_bound; the host meets the same bound against float64 in
    test_refine_host.py).  Measured on an MI355X: the device's S/N has the
    host's bits at both shapes (|device - host| / bound 0), and so the host's
    distance from float64, 0.115 and 0.081 of the bound."""
    from riptide_amd.refine import refine_host, refine_many
    g = rc.offset_job(B, S, N, K, J)
    assert list(g[3]) == [1, N // 3, N - 1] and g[4] == 1.7
    snr, prof = refine_many([g], profiles=True)[0]
    hsnr, hprof = refine_host(*g, profiles=True)
    assert np.array_equal(bits(prof), bits(hprof))
    _, f64, bound = rc.snr1_bound(hprof, g[3], g[4])
    snr, hsnr = (v.reshape(bound.shape).astype(np.float64) for v in (snr, hsnr))
    ratio, ratio64 = np.abs(snr - hsnr) / bound, np.abs(snr - f64) / bound
    print(f"device S/N with an offset {(B, S, N)}: largest |device - host| / bound {ratio.max():.3f}, "
          f"|device - float64| / bound {ratio64.max():.3f}")
    assert (ratio <= 1.0).all(), ratio.max()
    assert (ratio64 <= 1.0).all(), ratio64.max()


def test_unvalidated_device_tables(torch):
    """engine.refine_device does not validate device tables: entries of N,
    2N + 1, -1 and INT32_MIN run, as (v mod 2^32) mod N.  No value is illegal:
    the kernel reduces each entry as it loads it."""
    from riptide_amd import engine
    from riptide_amd.refine import pack_refine, refine_host
    B, S, N, K, J = 5, 4, 100, 3, 3
    g = job(B, S, N, K, J, "normal", seed=3)
    d, p = g[1].copy(), g[2].copy()
    d[1, :4] = [N, 2 * N + 1, -1, -2 ** 31]
    p[2, :4] = [-2 ** 31, -1, 2 * N + 1, N]
    cubes, shifts, widths, table, _, nsnr, nprof = pack_refine([(g[0], d, p, g[3], g[4])])
    dev = "cuda"
    snr, prof = engine.refine_device(torch.from_numpy(cubes).to(dev), torch.from_numpy(shifts).to(dev),
                                     torch.from_numpy(widths.astype(np.int32)).to(dev), table, profiles=True)
    torch.cuda.synchronize()
    assert snr.numel() == nsnr and prof.numel() == nprof

    def reduced(t):
        return ((t.astype(np.int64) % 2 ** 32) % N).astype(np.int32)
    hsnr, hprof = refine_host(g[0], reduced(d), reduced(p), g[3], g[4], profiles=True)
    assert np.array_equal(bits(prof.cpu().numpy().reshape(K, J, N)), bits(hprof))
    ok, msg = snr_close(snr.cpu().numpy().reshape(hsnr.shape), hsnr, rtol=1e-4)
    assert ok, msg
    snr2, none = engine.refine_device(torch.from_numpy(cubes).to(dev), torch.from_numpy(shifts).to(dev),
                                      torch.from_numpy(widths.astype(np.int32)).to(dev), table)
    assert none is None and torch.equal(snr2, snr)
    with pytest.raises(ValueError, match="exceed the device tensors"):
        engine.refine_device(torch.from_numpy(cubes[:-1]).to(dev), torch.from_numpy(shifts).to(dev),
                             torch.from_numpy(widths.astype(np.int32)).to(dev), table)


def test_host_buffer_form_validates(torch):
    from riptide_amd.refine import refine_many
    g = job(2, 3, 5, 2, 2, "int")
    for k, bad, text in ((1, 5, "DM shift outside"), (2, -1, "period shift outside")):
        t = g[k].copy()
        t[1, 1] = bad
        with pytest.raises(ValueError, match=text):
            refine_many([g[:k] + (t,) + g[k + 1:]])
    with pytest.raises(ValueError, match="trial widths must be all > 0 and < columns"):
        refine_many([g[:3] + ([1, 5], 1.0)])
    with pytest.raises(ValueError, match="stdnoise must be > 0"):
        refine_many([g[:4] + (0.0,)])
    with pytest.raises(ValueError, match="bins must be in"):
        refine_many([(np.zeros((1, 1, 1025), np.float32), [[0]], [[0]], [1], 1.0)])


def test_recovery_device(torch):
    """The CPU recovery case (test_refine_host.py) through the kernels: the
    same argmax."""
    from riptide_amd.refine import Refinement, refine_host, refine_many, refine_shifts
    periods, dms = rc.recovery_trials()
    pshift, dshift = refine_shifts(rc.R_PERIOD, rc.R_TOBS, rc.RN, rc.RS, rc.R_FREQS, rc.R_DM, periods, dms)
    jobs = [(rc.recovery_cube(seed, pshift, dshift), dshift, pshift, rc.R_WIDTHS, 8.0) for seed in range(4)]
    for g, snr in zip(jobs, refine_many(jobs)):
        r = Refinement(periods, dms, rc.R_WIDTHS, snr)
        h = Refinement(periods, dms, rc.R_WIDTHS, refine_host(*g))
        assert r.best_index[:2] == (rc.RK, rc.RJ) and r.best_index == h.best_index
        assert r.best_snr > r.snr_map[4, 4]


# ------------------------------------------------------------- from a file
F_PERIOD, F_DM, F_NSUB, F_BINS = 0.5, 20.0, 8, 64
F_RANGES = [{"name": "short",
             "ffa_search": {"period_min": 0.3, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
             "candidates": {"bins": F_BINS, "subints": 8}}]
F_DEREDDEN = {"rmed_width": 0.5, "rmed_minpts": 101}
# 8-sample pulses 6 units high over a channel noise of 10: folded over 65
# periods and a sub-band's 8 channels a bin of a sub-band holds the pulse at
# about 6 * 8 / 10 * sqrt(65 * 8 / 8) = 39 noise units, far above the trial to
# trial differences; the host specification is asserted on the same cube first
F_AMPLITUDE = 6.0
F_NOUT = 30000        # samples of every folded series: the largest delay here is a few hundred


def _pulse_filterbank(path):
    from test_gpu_dedisp import _write_filterbank
    nchans, nsamp = 64, 2 ** 15
    rng = np.random.RandomState(99)
    x = rng.normal(100.0, 10.0, size=(nsamp, nchans))
    sweep = dc.numpy_delays(dc.band(nchans), [F_DM], dc.TSAMP)[0]
    period = int(round(F_PERIOD / dc.TSAMP))
    for c in range(nchans):
        for t0 in range(100 + int(sweep[c]), nsamp - 8, period):
            x[t0:t0 + 8, c] += F_AMPLITUDE
    return _write_filterbank(path, np.clip(np.round(x), 0, 255).astype(np.uint8))


def test_refine_from_a_file(torch, tmp_path):
    import pandas  # noqa: F401  (Candidate.peaks is a DataFrame)
    from riptide_amd import Peak, PeakCluster, build_candidates_filterbank, refine_candidates
    from riptide_amd.dedispersion import band_edges
    from riptide_amd.reading import open_filterbank
    from riptide_amd.refine import default_trials
    fname = _pulse_filterbank(tmp_path / "r.fil")
    fb = open_filterbank(fname)
    band_freqs = np.array([fb.freqs[lo:hi].mean() for lo, hi in band_edges(fb.nchans, F_NSUB)])
    _, grid = default_trials(F_PERIOD, 30.0, F_BINS, band_freqs, F_DM)
    step = grid[1] - grid[0]
    dm0 = F_DM + 3.0 * step                  # the cluster: three default steps off the truth
    peak = Peak(period=F_PERIOD, freq=1.0 / F_PERIOD, width=3, ducy=3 / 64, iw=1, ip=0, snr=20.0, dm=dm0)
    plain = build_candidates_filterbank([PeakCluster([peak], rank=0)], fb, F_RANGES, F_DEREDDEN, nsub=F_NSUB,
                                        nout=F_NOUT)
    assert len(plain) == 1 and plain[0].refined is None            # the default is unchanged
    cands = build_candidates_filterbank([PeakCluster([peak], rank=0)], fb, F_RANGES, F_DEREDDEN, nsub=F_NSUB,
                                        nout=F_NOUT, refine=True)
    c = cands[0]
    assert c.subbands.shape == (F_NSUB, 8, F_BINS) and np.array_equal(c.subbands, plain[0].subbands)
    assert c.params["dm"] == dm0 and c.params["period"] == F_PERIOD

    def conditions(r):
        kc = int(np.argmin(np.abs(r.dms - dm0)))
        jc = int(np.argmin(np.abs(r.periods - F_PERIOD)))
        assert r.dms[kc] == dm0 and r.periods[jc] == F_PERIOD
        assert abs(r.best_dm - F_DM) < abs(dm0 - F_DM), (r.best_dm, dm0)
        assert abs(r.best_dm - F_DM) <= step * (1 + 1e-9), (r.best_dm, step)
        assert r.best_snr >= r.snr_map[kc, jc]

    # the host specification on the same cube meets the conditions ...
    host = refine_candidates([plain[0]], device=False, nsamp=F_NOUT)[0].refined
    conditions(host)
    # ... and so does the device
    dev = c.refined
    conditions(dev)
    assert np.array_equal(dev.dms, host.dms) and np.array_equal(dev.periods, host.periods)
    assert dev.snr.shape == (dev.dms.size, 33, dev.widths.size)
    ok, msg = snr_close(dev.snr, host.snr, rtol=1e-4)
    assert ok, msg
    assert dev.best_index == host.best_index and np.array_equal(bits(dev.profile), bits(host.profile))
