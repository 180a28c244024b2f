"""The scenes of tests/deepset.py do what tests/test_gpu_deep_levels.py relies on, from the oracle alone (no GPU): levels that grow with
depth up to the last of the 12 levels, a level that is exactly full, several packets and k_shade workgroups per level, both kinds of
child ray at every level, 33 shadow rays per hit.  Conditions, not measurements: a change to a scene that breaks one fails here."""
import numpy as np

import deepset

P = 1024                                      # primary rays of one tile: alloc_queues gives level d of a tile room for P << d rays
LEVELS = range(1, deepset.MAX_BOUNCES + 1)


def test_shells_doubles_its_rays_down_to_the_last_level():
    sc = deepset.shells()
    assert sc.tile_count == 1 and int(sc.config["bounces"][0]) == 11 and deepset.light_count(sc) == 2
    rays = deepset.level_rays(sc)
    print("shells rays per level", rays)
    assert len(rays) == 12 and rays[0] == P
    for d in LEVELS:
        assert rays[d] <= P << d, d                              # what the queue of the level holds
        assert 2 * rays[d] >= 3 * rays[d - 1], (d, rays)         # at least 1.5 x the level above
    assert rays[1] == P << 1                                     # exactly full
    assert 2 * rays[11] >= P << 11
    counts = deepset.level_counts(sc)
    assert all(counts[d]["reflection"] > 0 and counts[d]["refraction"] > 0 and counts[d]["shadow"] > 0 for d in LEVELS)
    frame = deepset.oracle_frame(sc)
    assert np.isfinite(frame["rgb"]).all()


def test_hall_keeps_every_level_busy_with_both_kinds_of_ray():
    sc = deepset.hall()
    assert sc.tile_count == 2 and len(sc.instances) == 2 and deepset.light_count(sc) == 3
    assert len(sc.point_lights) == 1 and len(sc.spot_lights) == 1 and len(sc.dir_lights) == 1
    counts, rays = deepset.level_counts(sc), deepset.level_rays(sc)
    print("hall rays per level", rays, "refraction", [c["refraction"] for c in counts])
    for d in LEVELS:
        assert rays[d] > 1024, (d, rays)
        assert rays[d] <= (2 * P) << d
        assert counts[d]["reflection"] > 0 and counts[d]["refraction"] > 0, (d, counts[d])
    assert np.isfinite(deepset.oracle_frame(sc)["rgb"]).all()


def test_hall_with_33_lights_casts_33_shadow_rays_per_lit_hit():
    few, many = deepset.hall(), deepset.hall(lights=33)
    assert (len(many.point_lights), len(many.spot_lights), len(many.dir_lights)) == (11, 11, 11)
    # the light list is the only thing that differs
    for a, b in ((few.spheres, many.spheres), (few.planes, many.planes), (few.instances, many.instances), (few.materials, many.materials),
                 (few.camera, many.camera), (few.config, many.config), (few.tlas_nodes, many.tlas_nodes)):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    # every material is lit wherever it is hit: a non-zero diffuse colour and no texture that could be black
    assert (np.asarray(many.materials["texture_id"])[1:] < 0).all()
    c3, c33 = deepset.level_counts(few), deepset.level_counts(many)
    for d in range(12):
        assert c33[d]["hits"] == c3[d]["hits"] > 0
        assert (c33[d]["reflection"], c33[d]["refraction"]) == (c3[d]["reflection"], c3[d]["refraction"])
        assert c33[d]["shadow"] == 33 * c33[d]["hits"], (d, c33[d])
        assert c3[d]["shadow"] == 3 * c3[d]["hits"]
    assert np.isfinite(deepset.oracle_frame(many)["rgb"]).all()
