#!/usr/bin/env python3
"""Writes tests/golden/branch_scenes.json: small scenes, each aimed at outcomes of the CPU oracle's path code that no
other parity scene takes (tests/oracle_coverage.py measures that; tests/test_oracle_branch_coverage.py is the gate).

Every scene is rows of this repository's own fixtures (fixtures.json, written by make_fixtures.js) with a few words
changed and, for most, another camera. The fixture holds data only: rows, a camera matrix, the frame shape, the
outcomes the scene is there for (`targets`: a copy of the oracle with that condition forced renders another frame) and
those it takes besides, on which no frame can depend (`also`), each as (function, condition text, outcome).

Two cameras do most of the work.
  * pencil(eye, target): a field of view of 1e-9 degrees. Every pixel and every jittered sample is the same ray to
    the bit (the pixel offsets are lost against the eye's coordinates), so one aimed ray is taken W * H * spp times,
    each time with its pixel's own hash sequence. This is how an exact pole hit or a grazing angle of 2e-5 is met
    more than once.
  * a camera further than MAX_DISTANCE from the rows, for the returns after a real root beyond that distance.

Usage: make_branch_scenes.py [out.json]   (needs the built package: the camera is sail_camera's)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from sail_amd import capi  # noqa: E402

with open(os.path.join(HERE, "fixtures.json")) as _f:
    FIX = json.load(_f)["scenes"]

MATTE = 1.0


def base(name):
    s = FIX[name]
    return {"objects": np.array(s["objects"], np.float64).reshape(s["n"], 18),
            "texparams": np.array(s["texparams"], np.float64).reshape(s["tn"], 16),
            "lights": np.array(s["lights"], np.float64).reshape(s["ln"], 18),
            "plugins": json.loads(json.dumps(s["plugins"])), "mvp_rowmajor": s["mvp_rowmajor"], "eye": list(s["eye"])}


def look(sc, eye, center, up=(0.0, 1.0, 0.0), fovy=55.0, znear=1.0, zfar=100.0):
    sc["eye"] = [float(v) for v in eye]
    sc["mvp_rowmajor"] = capi.camera(eye, center, up, fovy, 1.0, znear, zfar).tolist()


def f32(v):
    return float(np.float32(v))


def pencil(sc, eye, target, up=(0.0, 1.0, 0.0)):
    """near 1.5 and far 3 put the clip plane z = 0 two units from the eye with w = 1/2 exactly, so a coordinate of the
    eye that is an f32 comes back from the inverse matrix and the perspective divide as itself"""
    look(sc, [f32(v) for v in eye], [f32(v) for v in target], up, fovy=1e-9, znear=1.5, zfar=3.0)


def oren_nayar(tp, m, sigma=0.5):
    """texParams row m as an Oren-Nayar matte of roughness sigma (A and B as bsdf.glsl takes them)"""
    s2 = sigma * sigma
    tp[m][0], tp[m][2] = MATTE, sigma
    tp[m][3] = 1.0 - s2 / (2.0 * (s2 + 0.33))
    tp[m][4] = 0.45 * s2 / (s2 + 0.09)


def done(sc, W, H, spp, bounces, targets, also=()):
    o, t, l = sc["objects"], sc["texparams"], sc["lights"]
    return {"objects": [float(v) for v in o.reshape(-1)], "n": int(o.shape[0]),
            "texparams": [float(v) for v in t.reshape(-1)], "tn": int(t.shape[0]),
            "lights": [float(v) for v in l.reshape(-1)], "ln": int(l.shape[0]),
            "plugins": sc["plugins"], "mvp_rowmajor": sc["mvp_rowmajor"], "eye": sc["eye"],
            "W": W, "H": H, "spp": spp, "bounces": bounces, "targets": [list(t) for t in targets],
            "also": [list(t) for t in also]}


SCENES = {}

# ---- Cornell-set scenes (C1's three rows: 0 the light cube, 1 the Cornellbox, 2 the sphere; no light rows) --------------
# The pencil runs 4.99 units along z, 1e-4 above the floor at its start, and meets the floor at a slope of 2e-5:
# wo.z is about 2e-5, so sameHemisphere(wo, wi) = wo.z * wi.z > 1e-5 fails for the samples with wi.z < 0.5.
GRAZE_EYE, GRAZE_AT = (2.0, 1.0e-4, -6.5), (2.0, 0.0, -1.5)


def graze_lambert():
    sc = base("C1")
    pencil(sc, GRAZE_EYE, GRAZE_AT)
    return done(sc, 24, 16, 2, 6, [("matte", "sameHemisphere(wo, wi)  [1 of 2]", "false")])


def graze_oren_nayar():
    sc = base("C1")
    oren_nayar(sc["texparams"], 0)  # the box's (and the light's) material row
    pencil(sc, GRAZE_EYE, GRAZE_AT)
    return done(sc, 24, 16, 2, 6, [("matte", "sameHemisphere(wo, wi)  [2 of 2]", "false")])


# sphere local axes: x = -world z, y = world x, z = world y. Straight down its axis: hit.x == hit.y == 0 (the pole fix);
# down beside the axis in the plane z = centre z: hit.x == 0 alone.
def sphere_pole():
    sc = base("C1")
    c = sc["objects"][2][1:4]
    pencil(sc, (c[0], 5.0, c[2]), (c[0], 0.0, c[2]), up=(0.0, 0.0, 1.0))
    return done(sc, 24, 16, 2, 6, [], also=[("intersectSphere", "hit.x == F(0.0f)", "true"),
                                            ("intersectSphere", "hit.y == F(0.0f)", "true"),
                                            ("intersectSphere", "hit.x == F(0.0f) && hit.y == F(0.0f)", "true")])


def sphere_meridian():
    """ALL's glass sphere with the uv texture (only a texture makes phi matter), met beside its axis in the plane of
    its centre: hit.x == 0 and hit.y != 0"""
    sc = base("ALL")
    c = sc["objects"][3][1:4]
    pencil(sc, (c[0] + 0.2, 5.0, c[2]), (c[0] + 0.2, 0.0, c[2]), up=(0.0, 0.0, 1.0))
    return done(sc, 24, 16, 4, 8, [("intersectSphere", "hit.y == F(0.0f)", "false")])


def far_sphere():
    """C1 a thousand times larger, seen from 150,000 units: the sphere's nearer root lies beyond MAX_DISTANCE"""
    sc = base("C1")
    o = sc["objects"]
    o[0][1:7] *= 1000.0
    o[1][1:7] *= 1000.0
    o[2][1:5] *= 1000.0
    o[2][6] = 0.0                  # a matte
    o[2][8:11] = (3.0, 2.0, 1.0)    # that emits: a mutant that lets the hit through shows it
    look(sc, (2780.0, 2730.0, -150000.0), (2780.0, 2730.0, 0.0), fovy=2.4, znear=1000.0, zfar=400000.0)
    return done(sc, 24, 16, 2, 4, [], also=[("intersectSphere", "t >= F(kMaxDistance)", "true")])


def odd_rows_cornell():
    """C1 with three more rows whose category word no shape of the set has (negative, above 31, and a Cone's: AREA0's
    emitting cone, moved to the floor), and the sphere's material row index negative (the row coordinate's texel
    clamps to 0)"""
    sc = base("C1")
    o = sc["objects"]
    cone = base("AREA0")["objects"][3]
    cone[1:6] = (4.2, 0.0, 2.0, 2.0, 0.9)
    cone[7:9] = (0.0, 1.0)
    extra = np.stack([cone, cone, cone])
    extra[:, 0] = (-3.0, 40.0, 4.0)
    sc["objects"] = np.concatenate([o, extra])
    sc["objects"][2][6] = -2.0
    return done(sc, 32, 24, 4, 8, [("intersectObjects", "(C.shapeMask >> category) & 1u", "false"),
                                   ("texel", "!(s >= 0.0f)", "true")],
                also=[("intersectObjects", "category >= 0", "false"), ("intersectObjects", "category < 32", "false")])


# ---- scenes with light rows, textures, metal and glass --------------------------------------------------------------------
def emission_one_channel():
    """AREA's emitting mattes with emission (0, 0, e), (0, e, 0) and (e, 0, 0): veq's y and z comparisons decide (the
    registry's -0.0 emission rows already reach the y comparison)"""
    sc = base("AREA")
    o = sc["objects"]
    o[1][9:12] = (0.0, 0.0, 3.0)    # the disk
    o[2][8:11] = (0.0, 4.0, 0.0)    # the small sphere
    o[3][10:13] = (2.0, 0.0, 0.0)   # the rectangle
    o[4][8:11] = (0.0, 0.0, 0.5)    # the large sphere in the middle of the view
    return done(sc, 32, 24, 2, 5, [("veq", "a.z == b.z", "false")])


def far_quadrics():
    """AREA0 (one emitting row of every quadric kind) a thousand times larger, seen from 150,000 units"""
    sc = base("AREA0")
    o = sc["objects"]
    for r in o:
        cat = int(r[0])
        if cat in (1, 9):
            r[1:7] *= 1000.0
        elif cat == 2:
            r[1:5] *= 1000.0
        elif cat in (4, 5, 6):
            r[1:6] *= 1000.0
        elif cat == 7:
            r[1:10] *= 1000.0
            r[10:12] /= 1.0e6      # ah, ch: 1 / length^2
        elif cat == 8:
            r[1:7] *= 1000.0
    look(sc, (2780.0, 40000.0, -150000.0), (2780.0, 2730.0, 3000.0), fovy=2.4, znear=1000.0, zfar=400000.0)
    fns = ["intersectSphere", "intersectCone", "intersectCylinder", "intersectDisk", "intersectHyperboloid",
           "intersectParaboloid"]
    return done(sc, 48, 32, 2, 3, [], also=[(f, "t >= F(kMaxDistance)", "true") for f in fns])


def paraboloid_below_its_cut():
    """AREA0's paraboloid (apex (4.5, 4, 3), opening upward to y = 4.8) cut at z0 = 0.5. The ray starts outside above,
    crosses the uncut surface above the top (first root: out of range), runs through the bounding box and leaves
    through the surface below the cut (second root: out of range too)"""
    sc = base("AREA0")
    sc["objects"][6][4] = 0.5
    pencil(sc, (5.26, 5.4, 3.0), (4.3, 4.2, 3.0))
    return done(sc, 24, 16, 2, 4, [("intersectParaboloid", "hit.z < zMin  [2 of 2]", "true")])


# ALL: rows 0 the Cornellbox, 1 a matte sphere, 2 a metal sphere (material row 4), 3 a glass sphere (material row 6),
# 4 a disk on the floor (material row 8, texture row 9); a point and a spot light
def _disk_stage(mat_row):
    """ALL with its disk widened to radius 2.5 (no hole) and given material row mat_row"""
    sc = base("ALL")
    d = sc["objects"][4]
    d[4], d[5], d[7] = 2.5, 0.0, float(mat_row)
    return sc


def _graze_disk(sc, slope, side=1.0):
    """the pencil from 1e-4 above (side -1: below) the disk's plane, 1e-4 / slope away from where it lands (off the
    disk's centre)"""
    d = sc["objects"][4]
    run = 1.0e-4 / slope
    land = (d[1] + 0.7, d[2], d[3] + 0.4)
    pencil(sc, (land[0] - run, land[1] + side * 1.0e-4, land[2]), land)


def metal_flip():
    """rough metal met at wo.z about 2e-5: the sampled half vector has cos < 0.5 for most samples, so wo.z * wh.z fails
    sameHemisphere and the half vector is turned over"""
    sc = _disk_stage(4)
    sc["texparams"][4][1:3] = (1.5, 1.5)
    _graze_disk(sc, 2.0e-5)
    return done(sc, 24, 16, 2, 6, [("trSampleWh", "!sameHemisphere(wo, wh)", "true")])


def metal_below_eps():
    """metal met at a slope of 5e-6: not `into`, the normal is turned, wo.z = -5e-6 < EPSILON"""
    sc = _disk_stage(4)
    _graze_disk(sc, 5.0e-6)
    return done(sc, 24, 16, 2, 6, [("microfacet_r_sample_f", "wo.z < F(kEps)", "true")])


def glass_graze():
    """rough glass met at wo.z about 5e-4: the transmission half returns at equalZero(wo.z)"""
    sc = _disk_stage(6)
    sc["texparams"][6][4:6] = (0.4, 0.4)
    _graze_disk(sc, 5.0e-4)
    return done(sc, 24, 16, 2, 6, [("microfacet_t_sample_f", "equalZero(wo.z)", "true")])


def glass_from_below():
    """rough glass met from below (not `into`: eta 1.5) at wo.z about 2e-3, just past equalZero: about a tenth of the
    half vectors refract the ray into a direction that stays on wo's side of the surface"""
    sc = _disk_stage(6)
    sc["texparams"][6][4:6] = (3.0, 3.0)
    _graze_disk(sc, 2.0e-3, side=-1.0)
    return done(sc, 32, 24, 4, 4, [("microfacet_t_f", "sameHemisphere(wo, wi)", "true")],
                also=[("microfacet_t_pdf", "sameHemisphere(wo, wi)", "true")])


def glass_one_smooth_axis():
    """glass with ur = 0, vr > 0 on one sphere and the reverse on another: not specular, alpha 0 on one axis"""
    sc = base("ALL")
    o, tp = sc["objects"], sc["texparams"]
    tp[6][4:6] = (0.0, 0.3)
    tp[2] = tp[6]
    tp[2][4:6] = (0.3, 0.0)
    o[1][6] = 2.0                   # the matte sphere's material row: now the second glass
    return done(sc, 32, 24, 2, 6, [("glass", "vr < F(kEps)", "false")])


def glass_very_rough():
    """glass of roughness 1000 met at 45 degrees: nearly every sampled half vector has cos^2 < 1e-5, where tan2Theta
    returns INFINITY and trD 0.001. trD's value cancels between f and the pdf but for its rounding, so kt is 1e-4: that
    keeps f |cos| / pdf under shade's clamp at 1. (No frame was found to depend on tan2Theta's return by itself: forced,
    it hands trD sin^2 / cos^2, which is below INFINITY only for cos^2 within a 1e-5th of 1e-5.)"""
    sc = _disk_stage(6)
    sc["texparams"][6][4:6] = (1000.0, 1000.0)
    sc["texparams"][6][1:3] = (1.0e-4, 1.0e-4)
    d = sc["objects"][4]
    land = (d[1] + 0.7, d[2], d[3] + 0.4)
    pencil(sc, (land[0] - 1.0, land[1] + 1.0, land[2]), land)
    return done(sc, 24, 16, 2, 6, [("trD", "t2 >= F(kInf)", "true")], also=[("tan2Theta", "cos2T < F(kEps)", "true")])


def odd_rows_lit():
    """AREA with object rows of absent categories that its area lights point at (their samples have pdf 0: most of the
    frame is NaN)"""
    sc = base("AREA")
    o, lt = sc["objects"], sc["lights"]
    extra = np.repeat(o[2:3], 3, axis=0)
    extra[:, 0] = (-3.0, 40.0, 4.0)          # negative, above 31, a Cone's (not among AREA's shapes)
    sc["objects"] = np.concatenate([o, extra])
    sc["lights"] = np.concatenate([lt[:1], lt[:1], lt[:1], lt[:1], lt[2:]])
    for i, row in enumerate((5, 6, 7)):
        sc["lights"][1 + i][1] = float(row)
    return done(sc, 32, 24, 2, 5, [], also=[("sampleGeometry", "category >= 0", "false"),
                                            ("sampleGeometry", "category < 32", "false")])


def masked_rectangle():
    """AREA without the rectangle plugin: its rectangle row is no shape (invisible), and the area light that points at
    it samples nothing (pdf 0: NaN where it is picked)"""
    sc = base("AREA")
    sc["plugins"]["shape"].remove("rectangle")
    return done(sc, 32, 24, 2, 5, [("sampleGeometry", "(C.shapeMask >> category) & 1u", "false")])


def unmasked_texture():
    """AREA with a Bilerp's category word on the large sphere's texture row; bilerp is not among its texture plugins"""
    sc = base("AREA")
    sc["texparams"][9][0] = 8.0
    return done(sc, 32, 24, 2, 5, [("getSurfaceColor", "!((C.texMask >> texCategory) & 1u)", "true")])


def odd_lights(first, last):
    """ALL with light rows whose category words (the first and the last row's are the ones read) are `first`, `last`"""
    sc = base("ALL")
    lt = sc["lights"]
    sc["lights"] = np.concatenate([lt[1:], lt[:1], lt[1:]])
    sc["lights"][0][0], sc["lights"][2][0] = first, last
    return sc


def odd_lights_range():
    """(neither outcome can change a frame: a category outside 0..31 matches no light kind either way)"""
    return done(odd_lights(-1.0, 50.0), 24, 16, 2, 5, [], also=[("light_sample", "lightCategory >= 0", "false"),
                                                                ("light_sample", "lightCategory < 32", "false")])


for _f in (graze_lambert, graze_oren_nayar, sphere_pole, sphere_meridian, far_sphere, odd_rows_cornell,
           emission_one_channel, far_quadrics, paraboloid_below_its_cut, metal_flip, metal_below_eps, glass_graze,
           glass_from_below, glass_one_smooth_axis, glass_very_rough, odd_rows_lit, masked_rectangle, unmasked_texture,
           odd_lights_range):
    SCENES[_f.__name__] = _f()


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "branch_scenes.json")
    with open(out, "w") as f:
        json.dump(SCENES, f, separators=(",", ":"))
        f.write("\n")
