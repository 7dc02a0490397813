"""What tests/test_gpu_media_domain.py rests on, checked without a GPU (tests/media_domain.py): the conditions on the
inputs from the truth alone, the exactness of the scalings, and the truth itself against closed forms that do not go
through the companion-matrix solver."""
import numpy as np
import pytest

import media_domain as md
import media_truth as mt
import profile_truth as pt
import solver_domain as sd
import weights_truth as wt

f32 = np.float32
UNIT = [(u, kind, scene) for kind in md.KINDS for scene in md.SCENES for u in md.unit_cells(kind)]


def _id(v):
    return sd.cell_id(v) if isinstance(v, sd.Cell) else str(v)


@pytest.mark.parametrize("u,kind,scene", UNIT, ids=_id)
def test_cells_have_the_rays_the_assertions_need(u, kind, scene):
    """Conditions on the inputs, from truth alone, at the GPU tests' 1,024 rays.  Measured over the unit cells: non-robust
    share at most 1.4 % (lines of sight), 5.6 % (segments, r/R >= 0.25), 11.7 % (segments, r/R = 0.02); robust rays with a
    chord at least 502, segments wholly inside a tube 29, closed by the window's end 506 (478 of the tail cell's 1,000),
    starting inside and meeting a wall 256, nested scenes with four or more interval ends 337."""
    tr = md.truth(u, kind, scene)
    print(sd.cell_id(u), kind, scene, md.conditions(tr, scene))
    md.check_inputs(u, kind, scene, tr)
    assert len(tr["o"]) == md.N and tr["chords"].shape == (md.n_tori(scene), md.N)
    assert not tr["robust"].flags.writeable and not tr["A"].flags.writeable


@pytest.mark.parametrize("kind", md.KINDS)
def test_the_tail_cell_has_them_too(kind):
    for scene in md.SCENES:
        c = md.TAIL_CELL
        md.check_inputs(sd.unit_of(c), kind, scene, md.truth(c, kind, scene, md.N_TAIL))


def _normal(a):
    """Finite, and zero or a normal FP32 number: a power of two passed through it exactly."""
    a = np.asarray(a, f32)
    return bool(np.all(np.isfinite(a)) and np.all((a == 0) | (np.abs(a) >= np.finfo(f32).tiny)))


@pytest.mark.parametrize("kind", md.KINDS)
def test_scaled_inputs_are_the_unit_cells_scaled_exactly(kind):
    """Rays, windows, media and tables of every cell are bit for bit the unit cell's times the power of two (the segment
    recipe included), and nothing comes near overflow or the subnormals; the truth of a cell IS its unit cell's."""
    for c in cells_and_tail(kind):
        u, tag = sd.unit_of(c), sd.cell_id(c)
        o, d, tmin, tmax = md.rays(c, kind)
        o0, d0, tmin0, tmax0 = md.rays(u, kind)
        s = md.t_scale(c, kind)
        assert o.dtype == d.dtype == f32 and _normal(o) and _normal(d), tag
        assert np.array_equal(o, o0 * f32(2.0 ** c.k)) and np.array_equal(o.astype(np.float64), o0.astype(np.float64) * 2.0 ** c.k), tag
        dj = c.j if kind == "los" else c.k + c.j
        assert np.array_equal(d, d0 * f32(2.0 ** dj)) and np.array_equal(d.astype(np.float64), d0.astype(np.float64) * 2.0 ** dj), tag
        assert tmin == tmin0 * s and tmax == tmax0 * s and f32(tmin) == tmin and f32(tmax) == tmax and _normal([tmin, tmax]), tag
        for scene in md.SCENES:
            for (C, R, r), (C0, R0, r0) in zip(md.geo_of(c, scene), md.geo_of(u, scene)):
                assert (C, R, r) == (tuple(x * 2.0 ** c.k for x in C0), R0 * 2.0 ** c.k, r0 * 2.0 ** c.k) and _normal(list(C) + [R, r, r * r]), tag
            for (e, sg), (e0, sg0) in zip(md.media_of(c, scene), md.media_of(u, scene)):
                assert e == tuple(x * 2.0 ** -c.k for x in e0) and sg == sg0 * 2.0 ** -c.k and _normal(list(e) + [sg]), tag
            for shape in md.SHAPES:
                for t, t0 in zip(md.tables_of(c, scene, shape), md.tables_of(u, scene, shape)):
                    assert t.dtype == f32 and t.shape == (17, 4) and _normal(t), tag
                    assert np.array_equal(t.astype(np.float64), t0.astype(np.float64) * 2.0 ** -c.k) and (t0[:, 3] > 0).all(), tag
            assert md.truth(c, kind, scene) is md.truth(u, kind, scene)


def cells_and_tail(kind):
    return md.cells(kind) + [md.TAIL_CELL]


def test_segments_share_their_rays_between_the_scenes():
    """Both scenes of a cell get the same rays (torus j in the nested scene is compared with torus j alone ray by ray)."""
    for kind in md.KINDS:
        for u in md.unit_cells(kind):
            one, two = md.truth(u, kind, "one"), md.truth(u, kind, "nested")
            assert np.array_equal(one["o"], two["o"]) and np.array_equal(one["d"], two["d"])
            assert np.array_equal(one["chords"][0], two["chords"][0])
            assert (one["tmin"], one["tmax"]) == (two["tmin"], two["tmax"])


# --- the truth against closed forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("centre", [(0.0, 0.0, 0.0), sd.FAR_CENTRE], ids=["origin", "far"])
@pytest.mark.parametrize("ratio", sd.RATIOS)
def test_the_equatorial_ray_through_the_centre_has_a_chord_of_4r(ratio, centre):
    """A ray in the torus' plane through its centre crosses the tube twice along a diameter of its circular section:
    chord 4r, whatever R, r, the start and the length of the direction — and glow L = e·(1 - exp(-4r·sigma))/sigma for the
    two pieces 2(R - r) apart with nothing between them."""
    r = float(f32(ratio))
    C = np.array(centre)
    for dist, dlen in ((4.0, 1.0), (100.0, 2.0 ** -10), (12.0, 2.0 ** 10)):
        o = (C + np.array([-dist * (1.0 + r), 0.0, 0.0])).astype(f32)[None, :]
        d = np.array([[dlen, 0.0, 0.0]], f32)
        (eps, sig), = md.MEDIA[:1]
        tr = md.truth_on(o, d, [(tuple(C), 1.0, r)], None, md.MEDIA[:1], 1e-3 / dlen, 1e6 * dist / dlen, 1.0 + r)
        assert tr["robust"].all() and tr["ends"][0] == 4
        np.testing.assert_allclose(tr["chords"][0, 0], 4.0 * r, rtol=1e-9)   # (o is rounded to FP32: t is off by its ulp, the chord is not)
        np.testing.assert_allclose(tr["T"][0], np.exp(-4.0 * r * sig), rtol=1e-9)
        np.testing.assert_allclose(tr["L"][0], np.array(eps) * -np.expm1(-4.0 * r * sig) / sig, rtol=1e-9)


@pytest.mark.parametrize("ratio", sd.RATIOS)
def test_the_axis_rays_have_their_closed_forms(ratio):
    """Rays parallel to the axis through the tube, on the three tube ratios of the grid: the chord is 2a, the profile
    e·(1 - x) with sigma 0 gives L = e·4a³/(3r²) at any step count, the three moments of the weights are axis_moments, and
    the single weights at 1,024 steps are the closed form.  Their bar: along such a ray a hat is quadratic in the height
    between its kinks, which two Gauss points integrate exactly; a sub-step of world length l that straddles a kink is off
    by at most l times the hat's variation in it, l·16·|dx/ds| <= l·32/r; hat k has three kinks, each met twice:
    192·l²/r.  Measured: 0.017 of that (5.9e-6 of the chord) on all three ratios."""
    tr, table, a = md.axis_case(ratio)
    r = tr["geo"][0][2]
    assert tr["robust"].all() and (a > 0.3 * r).all()
    np.testing.assert_allclose(tr["chords"][0], 2.0 * a, rtol=1e-9)
    want_L = md.AXIS_E[None, :] * (4.0 * a ** 3 / (3.0 * r * r))[:, None]
    moments = wt.axis_moments(a, r)
    np.testing.assert_allclose(wt.moments_of(wt.axis_closed_form(a, r)), moments, rtol=1e-12)
    for steps in md.STEPS:
        L, T = pt.same_rule(tr, [table], steps)
        np.testing.assert_allclose(L, want_L, rtol=1e-9)
        assert (T == 1.0).all()
        np.testing.assert_allclose(wt.moments_of(wt.same_rule(tr, steps)[0]), moments, rtol=1e-9)
    err = np.abs(wt.same_rule(tr, 1024)[0] - wt.axis_closed_form(a, r)).max(0)
    bar = 192.0 * (2.0 * a / 1024) ** 2 / r
    assert (err <= bar).all() and (bar < 1e-2 * 2.0 * a / 17).all(), (err / bar).max()   # (the bar: below 1 % of a mean weight)


def test_the_margins_of_media_truth_default_to_its_own():
    """The optional margins of media_truth's helpers: with nothing passed, today's absolute 1e-3 and 1e-4."""
    c = mt.case("nest3", "seg")
    again = mt.truth_of(c["o"], c["d"], c["geo"], c["axes"], c["media"], c["tmin"], c["tmax"], c["bound"], delta=1e-4, t_tol=1e-3, end_margin=1e-3)
    assert np.array_equal(again["robust"], c["robust"]) and np.array_equal(again["ends_clear"], c["ends_clear"])
    wider = mt.truth_of(c["o"], c["d"], c["geo"], c["axes"], c["media"], c["tmin"], c["tmax"], c["bound"], end_margin=[1e-2, 1e-3, 1e-3])
    assert wider["robust"].sum() < c["robust"].sum() and not (wider["robust"] & ~c["robust"]).any()
