"""The option table of the device library (blom_amd/csrc/api.hip: g_opts): every name the three setters accepted before the
table existed is still accepted by the same setter and by no other, the readable reals read back, the validators refuse in
their own words, and a step that the host-side checks refuse leaves nothing behind in the context."""
import ctypes as C

import pytest

from blom_amd.cases import make_case
from blom_amd import hostinit
from parity import STATE_FIELDS

pytestmark = pytest.mark.gpu

# the names each setter accepted when the setters were chains of string compares, in their order there
REAL_NAMES = """baclin batrop delt1 dlt mdv2hi mdv2lo mdv4hi mdv4lo mdc2hi mdc2lo vsc2hi vsc2lo vsc4hi vsc4lo cbar cb cwbdts cwbdls
wuv1 wuv2 wts1 wts2 wbaro bdmc1 bdmc2 iwdfac nubmin vland pref swamxd egc eggam eglsmn egmndf egmxdf egidfq rhiscf ri0 tkepf
bdml_logc brine_mlbase_frac trxday srxday trxdpt srxdpt trxlim srxlim sref area xmi rm0 rm5 niwgf niwbf niwlf ale_regrid_nudge_ts
ce tau_mlr tau_growing_hbl tau_decaying_hbl tau_growing_hml tau_decaying_hml lfmin cl mstar nstar wpup_min mlbl_max_ratio
ale_stab_fac_limit ale_dpvar_fac ale_smooth_diff_max ale_dpmin_interior""".split()
INT_NAMES = """timing nstep lstep nday_in_year itriag itrtke itrgls tkeadv tkeidf gls vcoord_tag ltedtp_opt bdmtyp iwdflg bdmldp
allwet csdiag eddf2d edsprs edanis redi3d edfsmo rhsctp edritp_opt edwmth_opt difest_live full_physics aptflx apsflx ditflx disflx
srxbal ntda barotp_fused barotp_tile eddtra_frozen pgf_uv_pair pgf_uv_ring kprof_sel mom_aw_split mom_force_aw convec_nsingle
cmn_nslope_nb pgf_reuse scan_reassoc pgf_copy_fused check_period barotp_persist barotp_block barotp_overlap barotp_rimbuf
barotp_arctic_fused barotp_arctic_persist cnsvdi arctic_strips use_graph overlap phys_dag mom_early_at lean_fluxes tmsmt_fold
tmsmt_ahead ale_upper_bndr_ord ale_lower_bndr_ord ale_k_range_plevel ale_dktzu ale_dktzl ale_density_pc_upper_bndr
ale_density_pc_lower_bndr ale_tracer_pc_upper_bndr ale_tracer_pc_lower_bndr ale_velocity_pc_upper_bndr ale_velocity_pc_lower_bndr
remap_fold remap_nfirst halo_overlap cmnfld1 diapfl_du live_slopes ndiff_surface_align ndiff_rec_per_face momtum_bs momtum_lds_pad
momtum_order momtum_chunks_a momtum_chunks_b diffus_shfl""".split() + ["l%dmi" % k for k in range(1, 6)]
STR_NAMES = """expcnf mommth pgfmth advmth cppm_compatibility cppm_limiting eitmth mlrttp mlrmth vcoord_type
ale_reconstruction_method ale_regrid_method ale_density_limiting ale_tracer_limiting ale_velocity_limiting bmcmth""".split()
# a word every string option takes
STR_VALUES = dict(expcnf="channel", mommth="enscon", pgfmth="geopotential", advmth="remap", cppm_compatibility="full",
                  cppm_limiting="monotonic", eitmth="gm", mlrttp="constant", mlrmth="fox08", vcoord_type="isopyc_bulkml",
                  ale_reconstruction_method="ppm", ale_regrid_method="nudge", ale_density_limiting="monotonic",
                  ale_tracer_limiting="monotonic", ale_velocity_limiting="monotonic", bmcmth="uc")
READABLE = ["baclin", "batrop", "delt1", "dlt", "pref", "wbaro", "area", "bdml_logc"]
SKIP = {"util1", "util2", "util3", "util4"}        # scratch planes shared between stages


def _context(cfg="chan_s", init=False, **overrides):
    from blom_amd.gpu import BlomGpu
    case = make_case(cfg, **overrides)
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm)
    gpu = BlomGpu(case.idm, case.jdm, case.kdm, case.ntr, nreg, dict(ip=ip, iu=iu, iv=iv, iq=iq))
    if init:
        hostinit.init_state(gpu, case)
    return gpu


class _Raw:
    """the three setters and the getter with their return codes and messages, no fallback in between"""

    def __init__(self, gpu):
        self.gpu, self.lib = gpu, gpu.lib

    def err(self):
        return self.lib.blomgpu_last_error(self.gpu.ctx).decode()

    def real(self, name, v=1.0):
        return self.lib.blomgpu_set_real(self.gpu.ctx, name.encode(), C.c_double(v))

    def int(self, name, v=1):
        return self.lib.blomgpu_set_int(self.gpu.ctx, name.encode(), C.c_int(v))

    def str(self, name, v="x"):
        return self.lib.blomgpu_set_str(self.gpu.ctx, name.encode(), v.encode())

    def get(self, name):
        v = C.c_double(0.0)
        return self.lib.blomgpu_get_real(self.gpu.ctx, name.encode(), C.byref(v))


def _table(lib):
    """the table's names by the entry point that sets them (blomgpu_option_name)"""
    names, buf, kind, k = {0: [], 1: [], 3: []}, C.create_string_buffer(64), C.c_int(0), 0
    while lib.blomgpu_option_name(k, buf, 64, C.byref(kind)) == 0:
        names[1 if kind.value == 2 else kind.value].append(buf.value.decode())      # (2: an integer stored as v != 0)
        k += 1
    return names


def test_every_name_is_known_to_its_own_setter_and_to_no_other():
    gpu = _context()
    raw = _Raw(gpu)
    table = _table(gpu.lib)
    assert sorted(table[0]) == sorted(REAL_NAMES) and len(REAL_NAMES) == 72
    assert sorted(table[1]) == sorted(INT_NAMES) and len(INT_NAMES) == 92
    assert sorted(table[3]) == sorted(STR_NAMES) and len(STR_NAMES) == 16
    setters = dict(real=(raw.real, "blomgpu_set_real"), int=(raw.int, "blomgpu_set_int"), str=(raw.str, "blomgpu_set_str"))
    own = [(nm, "real") for nm in REAL_NAMES] + [(nm, "int") for nm in INT_NAMES] + [(nm, "str") for nm in STR_NAMES]
    for nm, kind in own + [("no_such_option", None)]:
        for other, (call, prefix) in setters.items():
            if other == kind:
                continue
            assert call(nm) != 0, (nm, other)
            assert raw.err() == f"{prefix}: unknown option {nm}", (nm, other)
        if nm not in READABLE:
            assert raw.get(nm) != 0 and raw.err() == f"blomgpu_get_real: unknown option {nm}", nm
    for nm in REAL_NAMES:
        assert raw.real(nm, 1.0) == 0, (nm, raw.err())
        gpu.set(nm, 1)                                     # an integer for a real option: set_int refuses, set_real takes it (gpu.py)
    for nm in INT_NAMES:
        assert raw.int(nm, 0 if nm == "barotp_tile" else 1) == 0, (nm, raw.err())
    for nm in STR_NAMES:
        assert raw.str(nm, STR_VALUES[nm]) == 0, (nm, raw.err())
    gpu.close()


def test_readable_reals_return_what_was_set():
    gpu = _context()
    for k, nm in enumerate(READABLE):
        v = 1.25 + 0.5 * k
        gpu.set(nm, v)
        assert gpu.get_real(nm) == v, nm
    for k, nm in enumerate(READABLE):                      # ... each its own, none through another's member
        assert gpu.get_real(nm) == 1.25 + 0.5 * k, nm
    gpu.close()


def test_validators_refuse_in_their_own_words_and_keep_the_old_value():
    """The five refusals, each with the message it has always had.  None of the five values can be read back, so `the old value stays in
    force` is checked through the results: a context that set valid values and was then refused five times steps to the same bytes as
    one that only set the valid values -- and, for mommth, to other bytes than one with the default, which a refusal that stored
    something (or fell back to the default) would not."""
    valid = dict(barotp_tile=3208, edritp_opt=1, l3mi=5, mommth="enecon", ale_density_limiting="monotonic")

    def run(refuse, **opts):
        gpu = _context(init=True)
        for k, v in opts.items():
            gpu.set(k, v)
        if refuse:
            raw = _Raw(gpu)
            assert raw.int("barotp_tile", 1234) != 0
            assert raw.err() == "blomgpu_set_int: barotp_tile must be 0, 3216, 3208, 1608, 4016, 2616, 2615 or 4015"
            assert raw.int("edritp_opt", 3) != 0 and raw.err() == " readnml_diffusion: edritp is unsupported!"
            assert raw.int("l3mi", 13) != 0 and raw.err() == "blomgpu_set_int: l3mi is a month, 1..12"
            assert raw.str("mommth", "foo") != 0 and raw.err() == " mommth = foo is unsupported!"
            assert raw.str("ale_density_limiting", "non_oscillatory") != 0
            assert raw.err() == " readnml_ale_regrid_remap: density_limiting = non_oscillatory is unsupported!"
        assert gpu.step(0, 2) == 2
        out = {nm: gpu.get(nm) for nm in STATE_FIELDS if gpu.has_field(nm) and nm not in SKIP}
        gpu.close()
        return out

    a, b, c = run(True, **valid), run(False, **valid), run(False)
    assert not [nm for nm in a if a[nm].tobytes() != b[nm].tobytes()]
    assert a["u"].tobytes() != c["u"].tobytes()


def test_refused_step_leaves_no_trace():
    """check_tracer_options refuses advmth = 'cppm' with tkeadv = 0 on the host, in front of the first launch of the step: the
    sequence's one way out has to leave the context as a fresh one"""
    def run(refused_first):
        gpu = _context("chan_s_tke", init=True, advmth="cppm")
        if refused_first:
            gpu.set("tkeadv", 0)
            with pytest.raises(Exception, match="tkeadv = 0 only with advmth = 'remap'"):
                gpu.step(0, 1)
            gpu.set("tkeadv", 1)
        assert gpu.step(0, 3) == 3
        out = {nm: gpu.get(nm) for nm in STATE_FIELDS if gpu.has_field(nm) and nm not in SKIP}
        gpu.close()
        return out

    a, b = run(True), run(False)
    assert len(a) > 40
    bad = [nm for nm in a if a[nm].tobytes() != b[nm].tobytes()]
    assert not bad, bad
