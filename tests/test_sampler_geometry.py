"""The production rig's env sampler (tests/production_rig.py sample_parts / sample_envs) pinned on hand-worked cases: which envs
it checks is only worth something if it follows the grid of the kernel under test (csrc/sdc_sweep.hpp first_pair_of_block, the
launches in csrc/sdc_capi.hip sdc_step).  No GPU needed.

Worked by hand:
  * lane per env (64 envs per workgroup of two wavefronts, four workgroups per CU = 1024 per round; sdc_capi.hip launch_step:
    128 sweep workgroups from 4096 envs up): 7 680 envs = 120 workgroups (a multiple of 8: XCD remap b -> (b % 8) * 15 + b // 8,
    the last workgroup stays last), 248 in the grid, one round; 7 744 envs = 121 workgroups (identity); 65 536 envs = 1024
    workgroups + 128 sweeps: dispatch slot 1024 is env workgroup 896, remapped to block 112; 262 144 envs = 4096 workgroups, 4 x 1024
    (DESIGN.md's "four dispatch rounds"), remap b -> (b % 8) * 512 + b // 8;
  * four envs per wavefront (16 envs per workgroup of four wavefronts, three per CU = 768 per round, max(32, N / 128) sweeps):
    5 636 envs = 353 workgroups (the last holds envs 5632..5635: a quarter full), 44 sweeps, one round; 7 616 envs = 476 (not a
    multiple of 8: identity), 59 sweeps;
  * two envs per wavefront, odd N: 7 681 envs = 961 workgroups of 8, the last holds env 7680 alone (a half-filled wavefront)."""
import numpy as np
import pytest

from tests.production_rig import CUS, GEOMETRY, env_block_of_workgroup, sample_envs, sample_parts

WIDE, QUAD = GEOMETRY["wide"], GEOMETRY["quad"]
LANES = (0, 1, 31, 32, 62, 63)


def _wide_block(b, vb, N, parts):
    assert parts["rounds"][b] == [vb * 64 + j for j in LANES], (N, b)


def test_first_pair_of_block_restated():
    assert [env_block_of_workgroup(b, 120) for b in (0, 1, 7, 8, 119)] == [0, 15, 105, 1, 119]
    assert [env_block_of_workgroup(b, 121) for b in (0, 1, 7, 8, 120)] == [0, 1, 7, 8, 120]
    assert [env_block_of_workgroup(b, 476) for b in (0, 1, 475)] == [0, 1, 475]
    remap = [env_block_of_workgroup(b, 4096) for b in range(4096)]
    assert sorted(remap) == list(range(4096)) and remap[1] == 512 and remap[8] == 1


@pytest.mark.parametrize("N,blocks,sweeps", [(7680, 120, 128), (7744, 121, 128), (65536, 1024, 128), (262144, 4096, 128)])
def test_wide_grid(N, blocks, sweeps):
    assert (WIDE.envs_per_wg, WIDE.envs_per_wave, WIDE.waves_per_wg, WIDE.wgs_per_cu) == (64, 64, 2, 4)
    assert WIDE.env_blocks(N) == blocks and WIDE.sweep_blocks(N) == sweeps
    p = sample_parts(N, WIDE)
    # every env (lane) of the first and the last env workgroup: both wavefronts of a workgroup serve the same 64 envs
    assert p["first"] == list(range(64)) and p["last"] == list(range(N - 64, N))


def test_wide_single_round_batches_have_no_boundary():
    assert sample_parts(7680, WIDE)["rounds"] == {} and sample_parts(7744, WIDE)["rounds"] == {}


def test_wide_65536_round_boundary():
    p = sample_parts(65536, WIDE)
    # dispatch slot 1024 = env workgroup 1024 - 128 = 896 (block 0 * 128 + 112), its predecessor 895 (block 7 * 128 + 111 = 1007);
    # env workgroup 1023 (the sweeps' slots handed on) is the last block; 1024 does not exist
    assert sorted(p["rounds"]) == [895, 896, 1023]
    _wide_block(895, 1007, 65536, p)
    _wide_block(896, 112, 65536, p)
    _wide_block(1023, 1023, 65536, p)


def test_every_cu_step_is_sampled():
    # a workgroup per CU more every 256 env workgroups: 65 536 envs on the lane-per-env kernel (remap b -> (b % 8) * 128 + b // 8)
    p = sample_parts(65536, WIDE)
    want = {255: 927, 256: 32, 511: 959, 512: 64, 767: 991, 768: 96}
    assert sorted(p["cu_steps"]) == sorted(want)
    for b, vb in want.items():
        assert p["cu_steps"][b] == [vb * 64 + j for j in LANES], b
    # 5 636 envs on the four-per-wavefront kernel (353 workgroups, identity): 255 | 256; 4096 envs, two per wavefront: 255 | 256 (511,
    # the last workgroup, is sampled whole anyway)
    assert sample_parts(5636, QUAD)["cu_steps"] == {255: [4080 + j for j in (0, 3, 4, 7, 8, 11, 12, 15)],
                                                    256: [4096 + j for j in (0, 3, 4, 7, 8, 11, 12, 15)]}
    # (512 workgroups of 8 envs, remap b -> (b % 8) * 64 + b // 8: 255 -> block 479, 256 -> 32; every env of each)
    pair = sample_parts(4096, GEOMETRY["pair"])
    assert pair["cu_steps"] == {255: list(range(3832, 3840)), 256: list(range(256, 264))} and pair["last"] == list(range(4088, 4096))
    assert sample_parts(7680, WIDE)["cu_steps"] == {}


def test_wide_262144_four_rounds():
    N = 262144
    assert WIDE.env_blocks(N) == 4 * CUS * WIDE.wgs_per_cu          # four dispatch rounds
    p = sample_parts(N, WIDE)
    want = {895: 3695, 896: 112, 1023: 3711, 1024: 128, 1919: 3823, 1920: 240, 2047: 3839, 2048: 256, 2943: 3951, 2944: 368,
            3071: 3967, 3072: 384, 3967: 4079, 3968: 496, 4095: 4095}
    assert sorted(p["rounds"]) == sorted(want)
    for b, vb in want.items():
        _wide_block(b, vb, N, p)
    s = sample_envs(N, WIDE, np.random.default_rng(5), n_random=64)
    assert set(range(64)) <= set(s) and set(range(N - 64, N)) <= set(s) and {112 * 64 + 63, 3695 * 64 + 31} <= set(s)
    assert len(s) >= 64 + 64 + 14 * 6 + 60


@pytest.mark.parametrize("N,blocks,sweeps,last", [(5636, 353, 44, list(range(5632, 5636))), (7616, 476, 59, list(range(7600, 7616)))])
def test_quad_grid(N, blocks, sweeps, last):
    assert (QUAD.envs_per_wg, QUAD.envs_per_wave, QUAD.wgs_per_cu) == (16, 4, 3)
    assert QUAD.env_blocks(N) == blocks and QUAD.sweep_blocks(N) == sweeps
    p = sample_parts(N, QUAD)
    assert p["first"] == list(range(16)) and p["last"] == last and p["rounds"] == {}


def test_quad_32768_round_boundaries():
    # 2048 workgroups + 128 sweeps, 768 per round: slots 768 and 1536 = env workgroups 640 / 1408, and 768 / 1536 themselves;
    # remap b -> (b % 8) * 256 + b // 8; a boundary workgroup is checked at the first and last env of each of its wavefronts
    p = sample_parts(32768, QUAD)
    want = {639: 1871, 640: 80, 767: 1887, 768: 96, 1407: 1967, 1408: 176, 1535: 1983, 1536: 192}
    assert sorted(p["rounds"]) == sorted(want)
    for b, vb in want.items():
        assert p["rounds"][b] == [vb * 16 + j for j in (0, 3, 4, 7, 8, 11, 12, 15)], b


def test_general_odd_batch_half_filled_last_wavefront():
    g = GEOMETRY["general"]
    assert g.env_blocks(7681) == 961 and g.sweep_blocks(7681) == 60
    p = sample_parts(7681, g)
    assert p["first"] == list(range(8)) and p["last"] == [7680]
    # 961 + 60 workgroups, 768 per round: env workgroups 707 | 708 and 767 | 768 (identity: 961 is odd), every env of each
    assert p["rounds"] == {707: list(range(5656, 5664)), 708: list(range(5664, 5672)), 767: list(range(6136, 6144)),
                           768: list(range(6144, 6152))}
