"""The critic on the CPU side (sdc_set_critic, sdc_critic_values, sdc_set_plan_critic, sdc_get_plan_critic): declared, exported and
bound with the ABI still at 313; sdc_critic_params' ctypes mirror has the C compiler's layout; a null handle is refused before any device
work; sdc_critic.hip cross-compiles for gfx950 with no scratch and no spills for exactly its two kernels; the host pack
(csrc/sdc_critic_pack.hpp, built into a small program by the host compiler alone) un-permutes to its input bit for bit, and a NumPy fp64
forward over the PACKED layout -- in the kernels' data flow -- agrees with tests/critic_ref.py on the unpacked network to 1e-12;
critic_params folds a ValueNorm as running_mean_var does and refuses a state_dict with a missing key."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import critic_ref as CR
from tests.plan_util import assert_c_layout, assert_no_scratch_or_spills, entry_point_header, kernel_resources

MEMBERS = ["ln0_g", "ln0_b", "w1", "b1", "ln1_g", "ln1_b", "w2", "b2", "ln2_g", "ln2_b", "w3", "b3", "scale", "shift", "flags"]


def test_entry_points_are_declared_exported_and_bound_at_abi_313():
    entry_point_header("sdc_set_critic", ["h", "p"], "sdc_critic.hip")
    entry_point_header("sdc_critic_values", ["h", "share_obs", "n_rows", "values", "stream"], "sdc_critic.hip")
    entry_point_header("sdc_set_plan_critic", ["h", "weight"], "sdc_critic.hip")
    entry_point_header("sdc_get_plan_critic", ["h", "weight"], "sdc_critic.hip")


def test_params_mirror_has_the_c_layout(tmp_path):
    assert_c_layout(tmp_path, "sdc_critic_params", L.SdcCriticParams, MEMBERS)
    assert L.SdcCriticParams.w1.size == 4 * 64 * 29 and L.SdcCriticParams.w2.size == 4 * 64 * 64 and L.SdcCriticParams.w3.size == 4 * 64


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    p, w = L.SdcCriticParams(), C.c_double(1.0)
    p.scale = 1.0
    assert lib.sdc_set_critic(None, C.byref(p)) == -2 and b"sdc_set_critic: null handle" in lib.sdc_last_error()
    assert lib.sdc_critic_values(None, None, 1, None, None) == -2 and b"sdc_critic_values: null handle" in lib.sdc_last_error()
    assert lib.sdc_set_plan_critic(None, 0.5) == -2 and b"sdc_set_plan_critic: null handle" in lib.sdc_last_error()
    assert lib.sdc_get_plan_critic(None, C.byref(w)) == -2 and b"sdc_get_plan_critic: null handle" in lib.sdc_last_error()
    assert w.value == 1.0


def test_critic_kernels_compile_for_gfx950_without_scratch_or_spills():
    per = kernel_resources("sdc_critic.hip")
    assert_no_scratch_or_spills(per, {"sdc_critic_values_kernel", "sdc_critic_terminal_kernel"})
    for k, u in per.items():      # (recorded in DESIGN.md section 4.24, not gated)
        print(k, "VGPRs", u.get("VGPRs"), "occupancy", u.get("Occupancy"), "LDS", u.get("LDS Size"))


# ---- the host pack -------------------------------------------------------------------------------------------------------------------
PACK_MAIN = r"""
#include <cstdio>
#include <memory>
#include "%s"
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::unique_ptr<sdc_critic_params> p(new sdc_critic_params);
  std::unique_ptr<SdcCriticDev> d(new SdcCriticDev);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(p.get(), sizeof(sdc_critic_params), 1, f) != 1) return 2;
  std::fclose(f);
  if (const char* why = sdc_critic_params_error(p.get())) {
    std::printf("%%s\n", why);
    return 3;
  }
  sdc_critic_pack(p.get(), d.get());
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(d.get(), sizeof(SdcCriticDev), 1, f) != 1) return 2;
  std::fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def pack_program(tmp_path_factory):
    """csrc/sdc_critic_pack.hpp behind a main(), built by the host compiler alone: params file -> packed file, or exit 3 and the reason"""
    td = tmp_path_factory.mktemp("critic_pack")
    src = td / "pack_main.cpp"
    src.write_text(PACK_MAIN % os.path.join(L.CSRC, "sdc_critic_pack.hpp"))
    exe = str(td / "pack_main")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-o", exe, str(src)], check=True)

    def run(params: L.SdcCriticParams):
        fin, fout = td / "params.bin", td / "packed.bin"
        fin.write_bytes(bytes(params))
        r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
        if r.returncode == 3:
            return r.stdout.strip()
        assert r.returncode == 0, r
        return CR.parse_packed(fout.read_bytes())

    return run


def _field(p, name):
    return np.ctypeslib.as_array(getattr(p, name)).copy()


@pytest.mark.parametrize("activation,feature_norm,value_norm", [("tanh", True, None), ("relu", False, CR.VALUE_NORM)])
def test_pack_unpermutes_to_its_input_and_the_packed_forward_is_the_network(pack_program, activation, feature_norm, value_norm):
    import torch
    from dc_rl_amd.engine import critic_params
    sd = CR.make_critic(7, feature_norm)
    p = critic_params(sd, value_norm, activation)
    d = pack_program(p)
    assert d["flags"] == p.flags == (1 if feature_norm else 0) | ((activation == "relu") << 1)
    u = CR.unpack(d)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert np.array_equal(bits(u["w1"][:, :29]), bits(_field(p, "w1").reshape(64, 29)))
    assert not u["w1"][:, 29:].any() and not u["ln0_g"][29:].any() and not u["ln0_b"][29:].any()      # (the padding is zero)
    assert np.array_equal(bits(u["w2"]), bits(_field(p, "w2").reshape(64, 64)))
    for name in ("b1", "ln1_g", "ln1_b", "b2", "ln2_g", "ln2_b", "w3"):
        assert np.array_equal(bits(u[name]), bits(_field(p, name))), name
    for name in ("ln0_g", "ln0_b"):
        assert np.array_equal(bits(u[name][:29]), bits(_field(p, name))), name
    for name in ("b3", "scale", "shift"):
        assert np.float32(d[name]) == np.float32(getattr(p, name)), name
    # every parameter of the generator is its own value: a swapped pair or a wrong unit would have shown above
    assert len(np.unique(_field(p, "w2"))) > 4000 and not np.array_equal(_field(p, "ln1_g"), _field(p, "ln1_b"))
    g = torch.Generator().manual_seed(3)
    x = torch.randn((16, 29), generator=g, dtype=torch.float64)
    ref = CR.forward(sd, x, activation, value_norm).numpy()
    got = CR.packed_forward(d, x.numpy(), activation)
    # (the restatement's scale is sqrt(var) in fp64, the struct's is fp32: compare in the struct's)
    if value_norm is not None:
        ref = (ref - value_norm[0]) / np.sqrt(value_norm[1]) * float(d["scale"]) + float(d["shift"])
    err = np.abs(got - ref).max()
    print("packed forward against the restatement: max |difference| %.2e" % err)
    assert err <= 1e-12, err


def test_pack_refuses_what_set_critic_refuses(pack_program):
    from dc_rl_amd.engine import critic_params
    good = critic_params(CR.make_critic(8))
    assert isinstance(pack_program(good), dict)

    def bad(**fields):
        p = L.SdcCriticParams.from_buffer_copy(bytes(good))
        for name, value in fields.items():
            if isinstance(value, tuple):
                getattr(p, name)[value[0]] = value[1]
            else:
                setattr(p, name, value)
        why = pack_program(p)
        assert isinstance(why, str), fields
        return why

    for x in (float("nan"), float("inf"), float("-inf")):
        assert "not finite" in bad(w1=(64 * 29 - 1, x)) and "not finite" in bad(ln0_g=(0, x)) and "not finite" in bad(b3=x)
        assert "not finite" in bad(shift=x)
    assert "not finite" in bad(scale=float("inf")) and "not finite" in bad(scale=float("nan"))
    assert "scale" in bad(scale=0.0) and "scale" in bad(scale=-1.0)
    assert "activation" in bad(flags=4) and "activation" in bad(flags=7)
    assert "flag" in bad(flags=8) and "flag" in bad(flags=-1)


# ---- critic_params -------------------------------------------------------------------------------------------------------------------
def test_critic_params_folds_a_value_norm_like_running_mean_var():
    import torch
    from dc_rl_amd.engine import critic_params, value_norm_scale_shift

    class ValueNorm:      # harl/common/valuenorm.py's three tensors after a few updates, and its own folding
        def __init__(self, mean, mean_sq, deb):
            self.running_mean = torch.tensor([mean], dtype=torch.float32)
            self.running_mean_sq = torch.tensor([mean_sq], dtype=torch.float32)
            self.debiasing_term = torch.tensor(deb, dtype=torch.float32)

        def running_mean_var(self):
            debiased_mean = self.running_mean / self.debiasing_term.clamp(min=1e-5)
            debiased_mean_sq = self.running_mean_sq / self.debiasing_term.clamp(min=1e-5)
            return debiased_mean, (debiased_mean_sq - debiased_mean ** 2).clamp(min=1e-2)

    sd = CR.make_critic(9)
    for vn in (ValueNorm(-0.031, 0.57, 0.0123), ValueNorm(2e-7, 3e-7, 1e-7), ValueNorm(0.5, 0.2501, 1.0), ValueNorm(0.0, 0.0, 0.0)):
        mean, var = vn.running_mean_var()
        want = (float(torch.sqrt(var)[0]), float(mean[0]))
        for form in (vn, dict(running_mean=vn.running_mean, running_mean_sq=vn.running_mean_sq, debiasing_term=vn.debiasing_term)):
            assert value_norm_scale_shift(form) == want
            p = critic_params(sd, form)
            assert (p.scale, p.shift) == (np.float32(want[0]), np.float32(want[1]))
    assert value_norm_scale_shift(None) == (1.0, 0.0)
    assert value_norm_scale_shift((-3.0, 56.25)) == (7.5, -3.0)
    p = critic_params(sd)
    assert (p.scale, p.shift, p.flags) == (1.0, 0.0, 1)
    assert critic_params(sd, activation="relu").flags == 3 and critic_params(CR.make_critic(9, feature_norm=False)).flags == 0
    # the struct's own fields are taken as they are
    fields = {k: sd[v] for k, v in CR.KEYS.items()}
    q = critic_params(dict(fields, scale=2.0, shift=-1.0, activation="relu"))
    assert bytes(q)[:L.SdcCriticParams.scale.offset] == bytes(p)[:L.SdcCriticParams.scale.offset]
    assert (q.scale, q.shift, q.flags) == (2.0, -1.0, 3)
    with pytest.raises(KeyError, match="running_mean"):
        critic_params(sd, {"mean": 0.0})


def test_critic_params_refuses_a_missing_key_a_wrong_shape_and_another_activation():
    from dc_rl_amd.engine import critic_params
    sd = CR.make_critic(10)
    for key in ("base.mlp.fc.0.weight", "base.mlp.fc.2.bias", "base.mlp.fc.3.bias", "base.mlp.fc.5.weight", "v_out.weight", "v_out.bias"):
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            critic_params({k: v for k, v in sd.items() if k != key})
    with pytest.raises(ValueError, match="w1"):
        critic_params(dict(sd, **{"base.mlp.fc.0.weight": sd["base.mlp.fc.0.weight"][:, :26]}))      # (an actor's width)
    with pytest.raises(NotImplementedError, match="selu"):
        critic_params(sd, activation="selu")
