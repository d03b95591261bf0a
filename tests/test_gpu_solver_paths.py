"""Every contact-solve path of the step kernel (tests/solver_paths.py) on the MI355X against the oracle: the first evaluation
and a short trajectory, in the generic kernel, the world-specific kernel where the world fits 64 KiB of LDS, two instances
per wavefront where the case is named for it, and - for the Vert cases whose QP uses the MFMA Gram product - the same
states again with the MFMA product switched off (rkfdDebugVariants(4)).  Every case first asserts, through the path helper
and the oracle's contact count, that it reaches the path it is named for."""
import pytest

import solver_paths as sp

B = 4
NSTEPS = 6
SPEC_LDS = 64 * 1024        # rkfdBatchSpecialize keeps the generic kernel above this


def _run(R, case, w, d, v, ors, kernel, what):
    b = R.Batch(w, B, device=0, max_rigid=case.cap)
    try:
        if kernel == "ipw2":
            b.set_instances_per_wave(2)
        if kernel in ("spec", "ipw2"):
            b.specialize()
        b.set_state(d, v)
        b.update_init()
        assert b.status() == 0
        e0 = sp.compare(b, ors, f"{what}: first evaluation")
        b.update(NSTEPS)
        assert b.status() == 0
        return e0, b
    except BaseException:
        b.close()
        raise


def _kernels(case, lds):
    if case.ipw == 2:
        return ["generic", "ipw2"]
    return ["generic", "spec"] if lds <= SPEC_LDS else ["generic"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sp.CASES, ids=sp.CASE_IDS)
def test_gpu_path_matches_oracle(R, tmp_path, case):
    w, dis, vel, _ = case.build(R, tmp_path)
    d, v = sp.states(dis, vel, B)
    lds = sp.devmodel_layout(w.model, case.cap)[3]
    variants = [0, 4] if case.tiles else [0]      # rkfdDebugVariants(4): the Vert QP's Gram product without MFMA
    worst = 0.0
    for mask in variants:
        for kernel in _kernels(case, lds):
            ors = sp.oracles(w, d, v)
            sp.check_path(R, case, w, ors[0], mask)
            what = f"{case.name} [{kernel}, variants {mask}]"
            R.lib().rkfdDebugVariants(mask)
            try:
                e0, b = _run(R, case, w, d, v, ors, kernel, what)
            finally:
                R.lib().rkfdDebugVariants(0)
            try:
                for o in ors:
                    o.update_n(NSTEPS)
                e1 = sp.compare(b, ors, f"{what}: {NSTEPS} steps")
            finally:
                b.close()
            worst = max(worst, e0, e1)
    print(f"{case.name}: nc {case.nc} max_rigid {case.cap} lds {lds} max rel err {worst:.2e}")


@pytest.mark.gpu
def test_gpu_rejects_a_world_over_the_lds_limit(R):
    """the Vert QP at a capacity of 32 needs more than 160 KiB of LDS per instance: refused at creation with a message; ten
    boxes at the largest MLCP capacity (42, 163 536 bytes) are accepted (case mlcp_grouped_full_nc40_lds_edge)"""
    w, *_ = sp.box_scene(R, ["flat"], solver="vert", pyramid=4)
    with pytest.raises(R.RkfdError, match="160 KiB"):
        R.Batch(w, 1, device=0, max_rigid=32)
    w10, *_ = sp.box_scene(R, ["flat"] * 10)
    b = R.Batch(w10, 1, device=0, max_rigid=42)
    assert b.lds_bytes == sp.devmodel_layout(w10.model, 42)[3] > sp.LDS_LIMIT - 1024
    b.close()
