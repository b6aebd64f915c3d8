"""What sdc_assign_envs writes from the host's copies of the configs (csrc/sdc_setup.hpp keeps them; nothing is read back from the
device): the CRAC set-point every env starts from is its own config's init_setpoint, 0.0 for a config that has not been set.  The
derived tables themselves are held bit for bit by tests/test_host_setup.py (without a GPU) and, on the device, by
tests/test_gpu_kernel_reach.py, test_gpu_wide_gen.py, test_gpu_production_sizes.py and test_gpu_snapshot.py."""
import numpy as np
import pytest

from dc_rl_amd import dc_config
from dc_rl_amd.engine import SdcEngine

pytestmark = pytest.mark.gpu


def test_assign_starts_every_env_from_its_configs_set_point():
    a = dc_config.size_datacenter("dc_config.json", 1)
    b = dict(dc_config.size_datacenter("dc_config_r16.json", 1), init_setpoint=20.5)
    assert a["init_setpoint"] == 18
    ids = np.array([0, 1, 2, 1, 0, 2], dtype=np.int32)      # config 2 is never set
    eng = SdcEngine(6, episode_steps=8, n_dc_configs=3)
    try:
        eng.assign(0, ids, 0, 364)      # before any config is set
        np.testing.assert_array_equal(eng.get_state("stpt"), np.zeros(6))
        np.testing.assert_array_equal(eng.get_state("cfg_id"), ids)
        eng.set_dc_params(0, a)
        eng.set_dc_params(1, b)
        eng.assign(0, ids, 0, 364)
        np.testing.assert_array_equal(eng.get_state("stpt"), np.array([18.0, 20.5, 0.0, 20.5, 18.0, 0.0]))
        eng.assign(0, ids[::-1].copy(), 0, 364)      # ... and follows a new assignment as long as no episode has started
        np.testing.assert_array_equal(eng.get_state("stpt"), np.array([0.0, 18.0, 20.5, 0.0, 20.5, 18.0]))
    finally:
        eng.close()
