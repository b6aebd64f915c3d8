"""Where a stepping call lands (csrc/sdc_dispatch.hpp), as the GPU tests have verified it on the device: the record that
tests/test_gpu_kernel_reach.py holds the library to and tests/test_step_dispatch.py holds the decision function to without a GPU.
A plain module: the test files import from here, not from one another.  Edit it on purpose when a threshold moves."""
from dc_rl_amd._lib import DEBUG_GENERAL as GENERAL
from dc_rl_amd._lib import DEBUG_PAIR as PAIR
from dc_rl_amd._lib import DEBUG_QUAD as QUAD
from dc_rl_amd._lib import DEBUG_WIDE as WIDE
from dc_rl_amd._lib import DEBUG_WIDE_OFF as WIDE_OFF

# single steps of a lock-step batch of one 20-rack config in the production configuration (debug_flags 0) -- odd N: general;
# N % 4 != 0: two envs per wavefront (pair); N % 4 == 0 from SDC_QUAD_MIN_ENVS_STEP = 5636: four per wavefront (quad); N % 64 == 0 from
# SDC_WIDE_MIN_ENVS = 7680: lane per env (wide); the ring's mirror from SDC_HIST_MIRROR_MIN_ENVS = 49152
KERNEL_OF_BATCH = {
    5632: "pair",        # the last size below the quad threshold
    5634: "pair",        # N % 4 != 0
    5636: "quad",        # the threshold itself; the last workgroup a quarter full (4 of 16 envs)
    7616: "quad",        # 476 workgroups: nb % 8 != 0, no XCD remap
    7680: "wide",        # the threshold itself
    7681: "general",     # odd: the last wavefront carries one env
    7682: "pair",
    7684: "quad",
    7744: "wide",        # 121 workgroups: nb % 8 != 0
    49088: "wide",       # the largest batch without the ring's mirror
    49216: "wide",       # with the mirror, 769 workgroups: nb % 8 != 0
}

KERNEL_NAME = {"general": "sdc_dynamics_kernel", "pair": "sdc_dynamics_fast_kernel", "quad": "sdc_dynamics_quad_kernel",
               "wide": "sdc_dynamics_wide_kernel", "wide_gen": "sdc_dynamics_wide_gen_kernel"}


def expected_mapping(flags, racks, classes, two_configs=False):
    """Where a 256-env batch lands (sdc_step): more than 32 racks -> the general kernel whatever the flags; the lane-per-
    env kernel's common form for one config of <= 8 classes (SDC_MAX_RACK_CLS), its general form up to 12 (SDC_WIDE_MAX_CLS) or for
    several configs, else two envs per wavefront; four envs per wavefront needs ONE config."""
    if racks > 32 or flags == GENERAL:
        return "general"
    if flags == QUAD and not two_configs:
        return "quad"
    if flags == WIDE:
        if classes <= 8 and not two_configs:
            return "wide"
        if classes <= 12:
            return "wide_gen"
    return "pair"


# (racks, rack classes or None: the shipped per-rack lists repeated)
RACK_CASES = [(1, None), (17, None), (31, None), (32, None), (33, None), (20, 8), (20, 9), (20, 12), (20, 13)]

# sdc_rollout over K = 3 steps of a small lock-step batch of the shipped 20-rack config: (envs, debug_flags, actions_out given) -> the
# kernel the call lands on.  Verified on the device against the library before the decision moved into sdc_dispatch.hpp.
ROLLOUT_CASES = [
    (256, 0, False, "sdc_rollout_fast_kernel"),
    (256, PAIR, False, "sdc_rollout_fast_kernel"),
    (256, QUAD, False, "sdc_rollout_quad_kernel"),
    (256, GENERAL, False, "sdc_rollout_kernel"),
    (256, WIDE, False, "sdc_dynamics_wide_kernel"),          # K single-step launches
    (256, 0, True, "sdc_rollout_kernel"),
    (256, WIDE, True, "sdc_dynamics_wide_gen_kernel"),       # K single-step launches of the kernel's general form
    (258, QUAD, False, "sdc_rollout_fast_kernel"),           # not a multiple of four
    (257, 0, False, "sdc_rollout_kernel"),                   # odd
]
