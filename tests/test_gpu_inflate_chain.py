"""The segment chain of the two-phase inflate is laid out twice: by
seg_chain_host (csrc/inflate_chain.h) and, for streams where every unit is on
the chain, by chain_kernel on the device (csrc/inflate_seg.hip).  Both get the
same hand-made unit tables here (zt_debug_chain / zt_debug_chain_host) and
must give the same chain units, segment jobs and totals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES_T = np.dtype([("out_len", "<u8"), ("end_bits", "<u8"), ("ntok", "<u4"), ("status", "<i4"), ("detail", "<i4"),
                  ("stop_idx", "<i4")])
# 1, 63, 64, 65: the edges of one wave round; 1025: 128 units per wave, two
# rounds; 8193: a second pass of the kernel's 8-round loop in wave 0
SIZES = [1, 63, 64, 65, 1025, 8193]


@pytest.fixture(scope="module")
def zt():
    import ztamd

    return ztamd


def tables(units, seed):
    """every unit on the chain: unit u stops at sync point u, the last at BFINAL"""
    rng = np.random.default_rng(seed)
    res = np.zeros(units, dtype=RES_T)
    res["out_len"] = rng.integers(0, 65536, units)
    res["out_len"][rng.random(units) < 0.1] = 0  # (the restart markers' empty units)
    res["end_bits"] = np.cumsum(rng.integers(8, 300000, units))
    direct = rng.random(units) < 0.3
    # runs of direct units, so that whole segments are direct too
    direct |= np.roll(direct, 1) & (rng.random(units) < 0.8)
    res["ntok"] = rng.integers(0, 1 << 16, units) | np.where(direct, 3 << 30, np.where(rng.random(units) < 0.5, 1 << 31, 0))
    res["stop_idx"] = np.arange(units)
    res["stop_idx"][-1] = -1
    # (at most about 1200 restart points: the kernel holds 2048 segments)
    restart = (rng.random(units - 1) < min(0.25, 600 / units)).astype(np.uint8)
    for k in range(units - 2):  # runs of consecutive restart points
        if restart[k] and rng.random() < 0.5:
            restart[k + 1] = 1
    tok_off = np.cumsum(rng.integers(64, 70000, units)).astype(np.uint64)
    return res, restart, tok_off


def caps(res, restart):
    total = int(res["out_len"].sum())
    max_seg = min(int(restart.sum()) + 1, len(res))
    return total, total + 512 * max_seg + 2048, max_seg


def compare(zt, res, restart, tok_off):
    out_cap, desc_cap, max_seg = caps(res, restart)
    hi, hcu, hsj = zt.debug_chain(res, restart, tok_off, out_cap, desc_cap, max_seg, host=True)
    di, dcu, dsj = zt.debug_chain(res, restart, tok_off, out_cap, desc_cap, max_seg)
    assert hi["outcome"] == 0 and hi["ok"] == 1
    assert di["ok"] == 1
    for k in ("nseg", "total", "end_bits", "desc_total"):
        assert di[k] == hi[k], k
    assert len(hcu) == len(res)
    for f in hcu.dtype.names:
        bad = np.nonzero(dcu[f] != hcu[f])[0]
        assert bad.size == 0, (f, int(bad[0]), int(dcu[f][bad[0]]), int(hcu[f][bad[0]]))
    for f in hsj.dtype.names:
        bad = np.nonzero(dsj[f] != hsj[f])[0]
        assert bad.size == 0, (f, int(bad[0]), int(dsj[f][bad[0]]), int(hsj[f][bad[0]]))
    return hi, hcu, hsj


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("units", SIZES)
def test_device_chain_is_the_host_chain(zt, units, seed):
    res, restart, tok_off = tables(units, 100 * units + seed)
    info, cu, sj = compare(zt, res, restart, tok_off)
    # (the tables do exercise what they are meant to)
    assert info["total"] == int(res["out_len"].sum())
    if units >= 63:
        assert info["nseg"] > 1
        assert (sj["count"] >> 31).any() and not (sj["count"] >> 31).all()
        assert (((cu["ntok"] >> 30) & 3) == 3).any()


def test_restart_at_unit_zero_and_all_direct(zt):
    res, restart, tok_off = tables(65, 7)
    restart[:3] = 1  # restart points right at the start: empty segments merge into the next
    res["out_len"][:3] = 0
    res["ntok"] |= 3 << 30
    info, cu, sj = compare(zt, res, restart, tok_off)
    assert (sj["count"] >> 31).all()


def invalid(zt, res, restart, tok_off):
    out_cap, desc_cap, max_seg = caps(res, restart)
    info, _, _ = zt.debug_chain(res, restart, tok_off, out_cap + (1 << 20), desc_cap + (1 << 20), max_seg)
    return info


def test_a_status_in_the_middle_is_not_the_device_chains(zt):
    res, restart, tok_off = tables(65, 11)
    res["status"][31] = -102
    assert invalid(zt, res, restart, tok_off)["ok"] == 0


def test_a_unit_of_65536_bytes_is_not_the_device_chains(zt):
    res, restart, tok_off = tables(65, 12)
    res["out_len"][40] = 65536
    assert invalid(zt, res, restart, tok_off)["ok"] == 0


def test_a_skipped_candidate_is_not_the_device_chains(zt):
    res, restart, tok_off = tables(65, 13)
    res["stop_idx"][20] = 21  # unit 21 is a false candidate
    assert invalid(zt, res, restart, tok_off)["ok"] == 0
