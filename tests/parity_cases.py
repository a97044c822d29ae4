"""The frames that GPU tests compare bit for bit with the CPU oracle, as one list: (id, scene, W, H, spp, bounces).

Taken from the test modules themselves (their case tables and their module-level scene builders), not retyped, so the
registry and the tests cannot drift apart. tests/test_oracle_branch_coverage.py measures which outcomes of the oracle's
path code these frames reach (tests/oracle_coverage.py). Accumulation modes, launch shapes and kernel forms do not
change which path a pixel takes, so each distinct (scene, shape) is listed once."""
import json
import os

import test_fuzz_scenes as fuzz
import test_gpu_jit_values as jit_values
import test_gpu_parity as parity
import test_gpu_row_shading as row_shading
import test_sphere_defer_gpu as sphere_defer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "fixtures.json")) as _f:
    FIXTURES = json.load(_f)

def registry():
    fx, sc = FIXTURES, FIXTURES["scenes"]
    cases = []
    for name, w, h, spp, b in parity.CASES + parity.COVERAGE:
        cases.append((f"parity:{name}:{w}x{h}x{spp}x{b}", sc[name], w, h, spp, b))
    for label, eye, center in parity.VIEWS:
        cases.append((f"view:{label}", parity.view_scene(fx, eye, center), 33, 21, 3, 6))
    for variant in sorted(parity.LAST_BOUNCE_MATS):
        for b in (1, 3):
            cases.append((f"last_bounce:{variant}:{b}", parity.last_bounce_scene(fx, variant), 24, 20, 3, b))
    cases.append(("odd_category_words", parity.odd_category_scene(fx), 24, 20, 3, 6))
    for name in fuzz.NAMES:
        cases.append((f"fuzz:{name}", fuzz.SCENES[name], fuzz.W, fuzz.H, fuzz.SPP, fuzz.B))
    sd = sphere_defer
    for which in sd.ROW_VARIANTS:
        cases.append((f"sphere_defer:{which}", sd.row_variant(fx, which), sd.W, sd.H, sd.SPP, sd.B))
    jv = jit_values
    for which in jv.HOSTILE:
        cases.append((f"hostile:{which}", jv._hostile(fx, which), jv.W, jv.H, jv.SPP, jv.B))
    rs = row_shading
    for row, what in rs._EDGES:
        cases.append((f"row_edge:{row}:{what}", rs._edge(fx, row, what)[0], rs.W, rs.H, rs.SPP, rs.B))
    for which in rs.ROW_VARIANTS:
        cases.append((f"row_shading:{which}", rs.row_variant(fx, which), rs.W, rs.H, rs.SPP, rs.B))
    for spheres, cubes in ((2, 0), (1, 2)):
        cases.append((f"more_rows:{spheres}:{cubes}", rs._more_rows(fx, spheres, cubes), rs.W, rs.H, rs.SPP, rs.B))
    return cases
