"""Host-side mirror of the reference's stage interface on top of libblomgpu.so (ctypes).

`BlomGpu` offers exactly what blom_amd.hostinit / blom_amd.stepper drive (get/put/set/stage
and the integer masks), with the reference's stage names and (m,n,mm,nn,k1m,k1n) argument
meaning (phy/mod_blom_step.F90:89-253).  There is no CPU fallback: if the HIP library is
missing or no device is present, construction raises.
"""
import ctypes as C
import math
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BLOMGPU_LIB: another build of the same library (A/B timing of kernel variants, tools/); never a different implementation
LIB_PATH = os.environ.get("BLOMGPU_LIB") or os.path.join(_HERE, "lib", "libblomgpu.so")


class blomgpu_dims(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("idm", "jdm", "kdm", "nbdy", "itdm", "jtdm", "i0", "j0",
                                       "nreg", "ntr", "device")]


def load_library():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc, gfx950). "
                           "blom_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    lib.blomgpu_last_error.restype = C.c_char_p
    lib.blomgpu_last_error.argtypes = [C.c_void_p]
    return lib


class BlomGpuError(RuntimeError):
    pass


class BlomGpu:
    def __init__(self, idm, jdm, kdm, ntr, nreg, masks, device=0, itdm=None, jtdm=None, i0=0, j0=0):
        self.lib = load_library()
        self.idm, self.jdm, self.kdm, self.ntr, self.nreg = idm, jdm, kdm, ntr, nreg
        self.ni, self.nj = idm + 8, jdm + 8
        self.itdm, self.jtdm = itdm or idm, jtdm or jdm
        d = blomgpu_dims(idm, jdm, kdm, 4, itdm or idm, jtdm or jdm, i0, j0, nreg, ntr, device)
        self.ctx = C.c_void_p()
        rc = self.lib.blomgpu_create(C.byref(d), C.byref(self.ctx))
        if rc:
            raise BlomGpuError(self.lib.blomgpu_last_error(None).decode())
        self.masks = {k: np.ascontiguousarray(masks[k], dtype=np.int32) for k in ("ip", "iu", "iv", "iq")}
        self._chk(self.lib.blomgpu_set_masks(self.ctx, *[self.masks[k].ctypes.data_as(C.c_void_p)
                                                         for k in ("ip", "iu", "iv", "iq")]))
        self._info = {}

    def close(self):
        if self.ctx:
            self.lib.blomgpu_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise BlomGpuError(self.lib.blomgpu_last_error(self.ctx).decode())

    # -- fields -----------------------------------------------------------------------
    def field_info(self, name):
        if name not in self._info:
            nlev, isint = C.c_int(0), C.c_int(0)
            rc = self.lib.blomgpu_field_info(self.ctx, name.encode(), C.byref(nlev), C.byref(isint))
            if rc:
                raise KeyError(name)
            self._info[name] = (nlev.value, bool(isint.value))
        return self._info[name]

    def has_stage(self, name):
        return True

    def has_field(self, name):
        try:
            self.field_info(name)
            return True
        except KeyError:
            return False

    def get(self, name):
        nlev, isint = self.field_info(name)
        a = np.empty((nlev, self.nj, self.ni), dtype=np.int32 if isint else np.float64)
        self._chk(self.lib.blomgpu_download(self.ctx, name.encode(), a.ctypes.data_as(C.c_void_p), nlev))
        return a

    def put(self, name, arr):
        nlev, isint = self.field_info(name)
        a = np.ascontiguousarray(arr, dtype=np.int32 if isint else np.float64)
        a = a.reshape((-1, self.nj, self.ni))
        n = min(nlev, a.shape[0])
        self._chk(self.lib.blomgpu_upload(self.ctx, name.encode(), a.ctypes.data_as(C.c_void_p), n))

    # -- options ----------------------------------------------------------------------
    def set(self, name, v):
        if isinstance(v, str):
            self._chk(self.lib.blomgpu_set_str(self.ctx, name.encode(), v.encode()))
        elif isinstance(v, (bool, int, np.integer)):
            rc = self.lib.blomgpu_set_int(self.ctx, name.encode(), C.c_int(int(v)))
            if rc:
                self._chk(self.lib.blomgpu_set_real(self.ctx, name.encode(), C.c_double(float(v))))
        else:
            self._chk(self.lib.blomgpu_set_real(self.ctx, name.encode(), C.c_double(float(v))))

    # -- stages -----------------------------------------------------------------------
    def stage(self, name, m, n, mm, nn, k1m, k1n):
        self._chk(self.lib.blomgpu_stage(self.ctx, name.encode(), m, n, mm, nn, k1m, k1n))

    def xctilr(self, name, lev0, l1, ld, mh, nh, itype):
        self._chk(self.lib.blomgpu_xctilr(self.ctx, name.encode(), lev0, l1, ld, mh, nh, itype))

    def set_vector(self, name, v):
        """1-D module arrays of the reference ("plevel", phy/mod_vcoord.F90:99)"""
        a = np.ascontiguousarray(v, dtype=np.float64)
        self.lib.blomgpu_set_vector.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int]
        self._chk(self.lib.blomgpu_set_vector(self.ctx, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))

    def step(self, nstep, nsteps=1):
        ns = C.c_int(nstep)
        self._chk(self.lib.blomgpu_step(self.ctx, C.byref(ns), nsteps))
        return ns.value

    def keep_flux_diagnostics(self, on=1):
        """on: every step of a step() call keeps utflx .. vsflx, u|v t|s fltd, u|v t|s flld current, not only its last two
        (get_real("flux_diag_steps_skipped") counts the steps that did not) -- blomgpu_keep_flux_diagnostics"""
        self._chk(self.lib.blomgpu_keep_flux_diagnostics(self.ctx, C.c_int(int(on))))

    def sync(self):
        self._chk(self.lib.blomgpu_sync(self.ctx))

    def crc(self, name, lev0, nlev, itype=1):
        v = C.c_uint(0)
        self._chk(self.lib.blomgpu_crc(self.ctx, name.encode(), lev0, nlev, itype, C.byref(v)))
        return v.value

    def crc_strips(self, name, lev0, nlev, itype=1):
        """This tile's share of the decomposition-independent checksum (xccrc, phy/mod_xc.F90:2195-2322): (l0, strips)
        with strips[row, s] the CRC of its s-th own 9-column strip of the global rows; chain with tiles.chain_crc."""
        cap = self.jdm * ((self.idm + 8) // 9 + 2)
        out = np.zeros(cap, dtype=np.uint32)
        l0, ns = C.c_int(0), C.c_int(0)
        self._chk(self.lib.blomgpu_crc_strips(self.ctx, name.encode(), lev0, nlev, itype, out.ctypes.data_as(C.c_void_p),
                                              cap, C.byref(l0), C.byref(ns)))
        return l0.value, out[:self.jdm * ns.value].reshape(self.jdm, ns.value).copy()

    def field_names(self):
        """every registered field (reals, then integers): the arrays a whole state consists of"""
        names, buf, k = [], C.create_string_buffer(64), 0
        while self.lib.blomgpu_field_name(self.ctx, k, buf, 64) == 0:
            names.append(buf.value.decode())
            k += 1
        return names

    def xcsum(self, name, lev=1, itype=1):
        """xcsum (phy/mod_xc.F90:4116) of one level of a device field; p-grid mask: ips."""
        v = C.c_double(0.0)
        self._chk(self.lib.blomgpu_xcsum(self.ctx, name.encode(), lev, itype, C.byref(v)))
        return v.value

    def xcsum_batch(self, name, lev0, nlev, mask="ips"):
        """xcsum of nlev consecutive levels of a field at once, through the kernels thermf_cesm's sums take -- blomgpu_xcsum_batch"""
        out = np.zeros(nlev, dtype=np.float64)
        self._chk(self.lib.blomgpu_xcsum_batch(self.ctx, name.encode(), int(lev0), int(nlev), mask.encode(), out.ctypes.data_as(C.c_void_p)))
        return out

    # -- the coupled experiment (expcnf = 'cesm') --------------------------------------------
    def inifrc_cesm(self):
        """inifrc_cesm (cesm/mod_cesm.F90:175-200) and the declaration that the coupler's forcing exists: creates the _da pairs, hmlt
        frzpot mltpot ztx mty, the stream fields, ipwocn ... -- blomgpu_inifrc_cesm"""
        self._chk(self.lib.blomgpu_inifrc_cesm(self.ctx))
        self._info = {}

    def put_level(self, name, plane, lev):
        """one level (1-based) of a real field from one plane -- blomgpu_upload_level"""
        a = np.ascontiguousarray(plane, dtype=np.float64).reshape(self.nj, self.ni)
        self._chk(self.lib.blomgpu_upload_level(self.ctx, name.encode(), a.ctypes.data_as(C.c_void_p), int(lev)))

    def getfrc_cesm(self):
        """getfrc_cesm (cesm/mod_cesm.F90:202-263) -- blomgpu_getfrc_cesm"""
        self._chk(self.lib.blomgpu_getfrc_cesm(self.ctx))

    def cesm_nflxdi(self):
        """mod_forcing's nflxdi(48) -- blomgpu_cesm_nflxdi"""
        out = np.zeros(48, dtype=np.int32)
        self._chk(self.lib.blomgpu_cesm_nflxdi(self.ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    # -- the forced ocean-ice experiment (expcnf = 'ben02clim' / 'ben02syn' / 'single_column') --------
    def inifrc_ben02(self):
        """the declaration that the forced ocean-ice experiment's forcing exists: creates hicem hsnwm ustari tauxice tauyice iagem tsrfm
        ticem tsi dfl albw alb rnfins rnfres, the five _tda accumulators, ztx mty, ipwocn ... -- blomgpu_inifrc_ben02"""
        self._chk(self.lib.blomgpu_inifrc_ben02(self.ctx))
        self._info = {}

    def ben02_ntda(self):
        """mod_ben02's ntda: the steps thermf_ben02 has accumulated into the _tda planes -- blomgpu_ben02_ntda"""
        n = C.c_int(0)
        self._chk(self.lib.blomgpu_ben02_ntda(self.ctx, C.byref(n)))
        return n.value

    def ben02_reset_tda(self):
        """the five _tda planes and ntda to zero, as asflux leaves them -- blomgpu_ben02_reset_tda"""
        self._chk(self.lib.blomgpu_ben02_reset_tda(self.ctx))

    # -- the end of blom_step: updswa, fwbbal, chkvar (options "swamth", "sprfac", "chkvar"; the clock: "step_time") --------
    def iniswa(self, chl=None):
        """iniswa (phy/mod_swabs.F90:216-609) for the method set("swamth", ...) names -- blomgpu_iniswa.  chl: for the chlorophyll methods,
        the monthly concentration (12, nj, ni) with halos; uploaded as chl10c = log10(chl) where chl is positive, as the reference's
        array holds it after iniswa."""
        self._chk(self.lib.blomgpu_iniswa(self.ctx))
        self._info = {}
        if chl is not None:
            a = np.array(chl, dtype=np.float64)
            pos = a > 0.0
            a[pos] = [math.log10(v) for v in a[pos]]      # (the C library's log10, element by element: the reference's call)
            self.put("chl10c", a)

    def updswa(self):
        """updswa (phy/mod_swabs.F90:611-732); returns at once unless a chlorophyll method is declared -- blomgpu_updswa"""
        self._chk(self.lib.blomgpu_updswa(self.ctx))

    def fwbbal(self, m, n, mm, nn, k1m, k1n):
        """fwbbal (phy/mod_forcing.F90:361-441); returns at once unless sprfac is set -- blomgpu_fwbbal"""
        self._chk(self.lib.blomgpu_fwbbal(self.ctx, m, n, mm, nn, k1m, k1n))

    def chkvar(self, m, n, mm, nn, k1m, k1n):
        """chkvar (phy/mod_chkvar.F90:77-141): raises BlomGpuError with the reference's line for the first NaN or Inf in dp, temp, saln of
        time level n; returns at once unless the option chkvar is set -- blomgpu_chkvar"""
        self._chk(self.lib.blomgpu_chkvar(self.ctx, m, n, mm, nn, k1m, k1n))

    def exp(self, x):
        """exp() as the kernels evaluate it (blom_amd/csrc/exp_libm.h), elementwise."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        y = np.empty_like(x)
        self._chk(self.lib.blomgpu_exp(self.ctx, x.size, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)))
        return y

    def get_real(self, name):
        v = C.c_double(0.0)
        self._chk(self.lib.blomgpu_get_real(self.ctx, name.encode(), C.byref(v)))
        return v.value

    def pow(self, x, y):
        """pow() as the kernels evaluate it (blom_amd/csrc/pow_libm.h), elementwise."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        z = np.empty_like(x)
        self._chk(self.lib.blomgpu_pow(self.ctx, x.size, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)))
        return z

    def sin(self, x):
        """sin() as the kernels evaluate it (blom_amd/csrc/sin_libm.h), elementwise."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        z = np.empty_like(x)
        self.lib.blomgpu_sin.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self._chk(self.lib.blomgpu_sin(self.ctx, x.size, x.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)))
        return z

    def atan2(self, y, x):
        """atan2() as the kernels evaluate it (blom_amd/csrc/atan2_libm.h), elementwise."""
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        z = np.empty_like(x)
        self.lib.blomgpu_atan2.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.lib.blomgpu_atan2(self.ctx, x.size, y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)))
        return z

    def tke_const(self, name):
        """a derived constant of the TKE closure (phy/mod_tke.F90:133-160) as this library evaluates it"""
        v = C.c_double(0.0)
        if self.lib.blomgpu_tke_const(name.encode(), C.byref(v)):
            raise KeyError(name)
        return v.value

    def budget_sums(self, ncall, n, nn):
        """budget_sums (phy/mod_budget.F90:95); does nothing unless the option cnsvdi is set."""
        self._chk(self.lib.blomgpu_budget_sums(self.ctx, ncall, n, nn))

    def budget_get(self, which, ncall, n):
        v = C.c_double(0.0)
        which = which if isinstance(which, int) else {"sdp": 0, "tdp": 1, "trdp": 2, "tkedp": 3, "glsdp": 4}[which]
        self._chk(self.lib.blomgpu_budget_get(self.ctx, which, ncall, n, C.byref(v)))
        return v.value

    BUDGET_SUMS = ("sdp", "tdp", "trdp", "tkedp", "glsdp")
    BUDGET_FILES = ("salbud", "tembud", "tkebud", "glsbud", "trcbud", "trcbudtot")

    def budget_init(self):
        """budget_init (phy/mod_budget.F90:73): the global mass sum mass0; does nothing unless the option cnsvdi is set."""
        self._chk(self.lib.blomgpu_budget_init(self.ctx))

    def budget_output(self, m):
        """budget_output's sums sf tf trf (phy/mod_budget.F90:335-352) into the record of the step the option nstep names -- for a host
        that sequences the stages itself; step() with the option budget_step does it by itself."""
        self._chk(self.lib.blomgpu_budget_output(self.ctx, m))

    def budget_mass0(self):
        v = C.c_double(0.0)
        self._chk(self.lib.blomgpu_budget_mass0(self.ctx, C.byref(v)))
        return v.value

    def budget_steps(self):
        """(first step, number of steps) the library holds records of: the last step() call's and the one of the step before it"""
        first, count = C.c_int(0), C.c_int(0)
        self._chk(self.lib.blomgpu_budget_steps(self.ctx, C.byref(first), C.byref(count)))
        return first.value, count.value

    def budget_record(self, nstep):
        """the record of one step: the five sums of the seven calls as {name: array of 7}, sc, and sf tf trf as computed at its end"""
        r = np.zeros(39)
        self._chk(self.lib.blomgpu_budget_record(self.ctx, nstep, r.ctypes.data_as(C.c_void_p)))
        out = {nm: r[:35].reshape(7, 5)[:, q].copy() for q, nm in enumerate(self.BUDGET_SUMS)}
        out.update(sc=r[35], sf=r[36], tf=r[37], trf=r[38])
        return out

    def budget_records(self):
        """every record held, as a dict of arrays with the steps along the first axis (key "nstep": the step numbers)"""
        first, count = self.budget_steps()
        recs = [self.budget_record(first + k) for k in range(count)]
        out = {"nstep": np.arange(first, first + count)}
        for nm in self.BUDGET_SUMS + ("sc", "sf", "tf", "trf"):
            out[nm] = np.array([r[nm] for r in recs]) if recs else np.zeros((0, 7) if nm in self.BUDGET_SUMS else (0,))
        return out

    def budget_line(self, nstep, file):
        """the terms budget_output writes for step nstep into `file` (phy/mod_budget.F90:211-331); the file's first column is nstep - 1"""
        t, n = np.zeros(7), C.c_int(0)
        self._chk(self.lib.blomgpu_budget_line(self.ctx, nstep, self.BUDGET_FILES.index(file), t.ctypes.data_as(C.c_void_p), C.byref(n)))
        return t[:n.value].copy()

    def budget_files(self):
        """the files the tracer set calls for (phy/mod_budget.F90:231-268)"""
        mask = C.c_int(0)
        self._chk(self.lib.blomgpu_budget_files(self.ctx, C.byref(mask)))
        return [f for k, f in enumerate(self.BUDGET_FILES) if mask.value >> k & 1]

    def budget_lines(self):
        """{file: (nstep - 1 of every line, terms[line, term])} for the files the tracer set calls for and the steps that have a line"""
        first, count = self.budget_steps()
        out = {}
        for f in self.budget_files() if count else ():
            rows = [self.budget_line(s, f) for s in range(first + 1, first + count)]
            out[f] = (np.arange(first, first + len(rows)), np.array(rows).reshape(len(rows), 7 if f == "trcbudtot" else 6))
        return out

    # -- time-mean diagnostics (diaacc, phy/mod_dia.F90) -------------------------------------
    def dia_names(self):
        """the accumulator table: [(name, kind, grid)] with kind 0 = 2-D, 1 = kdm layers, 2 = ddm depth levels and grid one of
        "p", "u", "v" """
        rows, buf, k = [], C.create_string_buffer(32), 0
        lyr, grid = C.c_int(0), C.c_int(0)
        while self.lib.blomgpu_dia_name(k, buf, 32, C.byref(lyr), C.byref(grid)) == 0:
            rows.append((buf.value.decode(), lyr.value, "puv"[grid.value]))
            k += 1
        return rows

    def dia_names_all(self):
        """the whole table: the rows of dia_names() in their order, then the six density-class rows (kind 3: kdm classes) --
        blomgpu_dia_name_all"""
        rows, buf, k = [], C.create_string_buffer(32), 0
        kind, grid = C.c_int(0), C.c_int(0)
        while self.lib.blomgpu_dia_name_all(k, buf, 32, C.byref(kind), C.byref(grid)) == 0:
            rows.append((buf.value.decode(), kind.value, "puv"[grid.value]))
            k += 1
        return rows

    def dia_names_full(self):
        """the whole table: the rows of dia_names_all() in their order, then diavfl's -- wflx wflx2 (kind 1), wflxlvl wflx2lvl
        (kind 2) and the group's internal slots uflxold vflxold (kind 4: ddm depth levels, not selectable by name) --
        blomgpu_dia_name_full"""
        rows, buf, k = [], C.create_string_buffer(32), 0
        kind, grid = C.c_int(0), C.c_int(0)
        while self.lib.blomgpu_dia_name_full(k, buf, 32, C.byref(kind), C.byref(grid)) == 0:
            rows.append((buf.value.decode(), kind.value, "puv"[grid.value]))
            k += 1
        return rows

    def dia_names_ext(self):
        """the whole table: the rows of dia_names_full() in their order, then the column-derived rows -- sbot tbot t20d t17d mldl82
        mldl82mn mldl82mx mldl82sq (kind 0) and avdsg dpvor (kind 1) -- blomgpu_dia_name_ext"""
        rows, buf, k = [], C.create_string_buffer(32), 0
        kind, grid = C.c_int(0), C.c_int(0)
        while self.lib.blomgpu_dia_name_ext(k, buf, 32, C.byref(kind), C.byref(grid)) == 0:
            rows.append((buf.value.decode(), kind.value, "puv"[grid.value]))
            k += 1
        return rows

    def dia_names_msc(self):
        """the rows of dia_names_ext() in their order, then the 23 msc names that dia_reduce forms from the accumulators at output
        time (kind 5) -- blomgpu_dia_name_msc"""
        out, k = [], 0
        buf, kind, grid = C.create_string_buffer(32), C.c_int(0), C.c_int(0)
        while self.lib.blomgpu_dia_name_msc(k, buf, 32, C.byref(kind), C.byref(grid)) == 0:
            out.append((buf.value.decode(), kind.value, "puv"[grid.value]))
            k += 1
        return out

    def dia_set_mertra(self, mtlat=None, nind=None, pts=None, oflg=None, ocn_nreg=0, nflg=None, regflg=None, minlat=None, maxlat=None):
        """diamer's sections and regions (phy/mod_dia.F90:4026-4108): mtlat (lmax,), nind (lmax,), pts (sum nind, 4) = (i, j, uflg,
        vflg) 1-based global, oflg (jtdm, itdm), regflg (mer_nreg, 20) with nflg (mer_nreg,) and the latitude bounds; no argument
        clears the table -- blomgpu_dia_set_mertra"""
        if mtlat is None:
            self._chk(self.lib.blomgpu_dia_set_mertra(self.ctx, 0, None, None, None, None, 0, 0, None, None, None, None))
            return
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        mtlat, minlat, maxlat = f8(mtlat), f8(minlat), f8(maxlat)
        nind, pts, oflg, nflg, regflg = i4(nind), i4(pts).reshape(-1, 4), i4(oflg), i4(nflg), i4(regflg)
        if nind.size != mtlat.size or pts.shape[0] != int(nind.sum()) or regflg.shape != (nflg.size, 20) or minlat.size != nflg.size or maxlat.size != nflg.size:
            raise ValueError("dia_set_mertra: the tables' extents do not agree")
        if oflg.shape != (self.jtdm, self.itdm):
            raise ValueError(f"dia_set_mertra: oflg has shape {oflg.shape}, the global domain is (jtdm, itdm) = {(self.jtdm, self.itdm)}")
        self._chk(self.lib.blomgpu_dia_set_mertra(self.ctx, C.c_int(mtlat.size), p(mtlat), p(nind), p(pts), p(oflg), C.c_int(int(ocn_nreg)),
                                                  C.c_int(nflg.size), p(nflg), p(regflg), p(minlat), p(maxlat)))

    def dia_set_sections(self, nsi=None, pts=None, equat_sec=-1):
        """diasec's sections (phy/mod_dia.F90:3838-3866): nsi (sec_num,), pts (sum nsi, 4) = (i, j, usi, vsi), equat_sec the 1-based
        section of the upper-350 m sums or -1; no argument clears the table -- blomgpu_dia_set_sections"""
        if nsi is None:
            self._chk(self.lib.blomgpu_dia_set_sections(self.ctx, 0, None, None, -1))
            return
        nsi, pts = np.ascontiguousarray(nsi, dtype=np.int32), np.ascontiguousarray(pts, dtype=np.int32).reshape(-1, 4)
        if pts.shape[0] != int(nsi.sum()):
            raise ValueError("dia_set_sections: the tables' extents do not agree")
        self._chk(self.lib.blomgpu_dia_set_sections(self.ctx, C.c_int(nsi.size), nsi.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p),
                                                    C.c_int(int(equat_sec))))

    def dia_reduce(self):
        """diamer, diasec and the global sums for the selected msc names, in front of dia_finalize -- blomgpu_dia_reduce"""
        self._chk(self.lib.blomgpu_dia_reduce(self.ctx))

    def dia_msc(self, name):
        """one result of the last dia_reduce in the reference's shape: (mer_nreg, kdm | ddm, lmax), (mer_nreg, lmax), (sec_num,) or
        (1,) -- blomgpu_dia_msc_get"""
        dims = (C.c_int * 3)()
        self._chk(self.lib.blomgpu_dia_msc_get(self.ctx, name.encode(), None, 0, dims))       # cap = 0: the shape alone
        n = dims[0] * dims[1] * dims[2]
        a = np.empty(n)
        self._chk(self.lib.blomgpu_dia_msc_get(self.ctx, name.encode(), a.ctypes.data_as(C.c_void_p), n, dims))
        ndim = 3 if name.startswith("mm") else 2 if name[:2] in ("mh", "ms") else 1      # stream functions, transports, the others
        return a.reshape([dims[k] for k in range(ndim)])

    def dia_select(self, names):
        """replace the selection (a blank-separated string or a list of names; empty: none) -- blomgpu_dia_select"""
        if not isinstance(names, str):
            names = " ".join(names)
        self._chk(self.lib.blomgpu_dia_select(self.ctx, names.encode()))

    def diaacc(self, m, n, mm, nn, k1m, k1n):
        self._chk(self.lib.blomgpu_diaacc(self.ctx, m, n, mm, nn, k1m, k1n))

    def dia_nacc(self):
        v = C.c_int(0)
        self._chk(self.lib.blomgpu_dia_nacc(self.ctx, C.byref(v)))
        return v.value

    def dia_get(self, name):
        """the accumulator as get() would return a field: (1 | kdm | ddm, nj, ni)"""
        if not hasattr(self, "_dia_lyr"):
            self._dia_lyr = {nm: lyr for nm, lyr, _ in self.dia_names_ext()}
        if name not in self._dia_lyr:
            raise KeyError(name)
        nlev = (1, self.kdm, len(self.dia_levels()), self.kdm, len(self.dia_levels()))[self._dia_lyr[name]]
        a = np.empty((nlev, self.nj, self.ni), dtype=np.float64)
        self._chk(self.lib.blomgpu_dia_get(self.ctx, name.encode(), a.ctypes.data_as(C.c_void_p)))
        return a

    def dia_finalize(self):
        self._chk(self.lib.blomgpu_dia_finalize(self.ctx))

    def dia_reset(self):
        self._chk(self.lib.blomgpu_dia_reset(self.ctx))

    def dia_alarm(self, alarm):
        """declare the reference's output alarm alarm_phy(1), 0 or 1: under cntiso_hybrid / plevel templvl salnlvl uvellvl vvellvl take
        their sample inside ale_regrid_remap while it is 0 (phy/mod_ale_regrid_remap.F90:1524-1531) and in ale_remap_diazlv when it
        is 1 (:2014-2017) -- blomgpu_dia_alarm"""
        self._chk(self.lib.blomgpu_dia_alarm(self.ctx, C.c_int(int(alarm))))

    def ale_remap_diazlv(self, m, n, mm, nn, k1m, k1n):
        """the end-of-step sample of an output step (phy/mod_ale_regrid_remap.F90:1986-2201; phy/mod_blom_step.F90:271-273), with the
        indices of the step that has just returned -- blomgpu_ale_remap_diazlv"""
        self._chk(self.lib.blomgpu_ale_remap_diazlv(self.ctx, m, n, mm, nn, k1m, k1n))

    def dia_set_levels(self, bnds=None, levitus2x=False):
        """the depth levels of the *lvl names: bnds[ddm][2] (upper, lower bound in metres; increasing, contiguous), None for the
        default 35 levels, levitus2x=True for the reference's 70 -- blomgpu_dia_set_levels / blomgpu_dia_levels_levitus2x"""
        if levitus2x:
            self._chk(self.lib.blomgpu_dia_levels_levitus2x(self.ctx))
        elif bnds is None:
            self._chk(self.lib.blomgpu_dia_set_levels(self.ctx, None, 0))
        else:
            a = np.ascontiguousarray(bnds, dtype=np.float64).reshape(-1, 2)
            self._chk(self.lib.blomgpu_dia_set_levels(self.ctx, a.ctypes.data_as(C.c_void_p), C.c_int(a.shape[0])))

    def dia_levels(self):
        """the depth levels in force, (ddm, 2) -- blomgpu_dia_get_levels"""
        ddm = C.c_int(0)
        self._chk(self.lib.blomgpu_dia_get_levels(self.ctx, None, 0, C.byref(ddm)))
        a = np.empty((ddm.value, 2), dtype=np.float64)
        self._chk(self.lib.blomgpu_dia_get_levels(self.ctx, a.ctypes.data_as(C.c_void_p), ddm, C.byref(ddm)))
        return a

    def dia_set_sigdia(self, sigdia=None):
        """the kdm diagnostic density classes of the class names (umfll ...), None to clear the table -- blomgpu_dia_set_sigdia"""
        if sigdia is None:
            self._chk(self.lib.blomgpu_dia_set_sigdia(self.ctx, None, 0))
        else:
            a = np.ascontiguousarray(sigdia, dtype=np.float64).ravel()
            self._chk(self.lib.blomgpu_dia_set_sigdia(self.ctx, a.ctypes.data_as(C.c_void_p), C.c_int(a.size)))

    def dia_sigdia(self):
        """the density classes in force, (kdm,), or an empty array without a table -- blomgpu_dia_get_sigdia"""
        n = C.c_int(0)
        self._chk(self.lib.blomgpu_dia_get_sigdia(self.ctx, None, 0, C.byref(n)))
        a = np.empty(n.value, dtype=np.float64)
        self._chk(self.lib.blomgpu_dia_get_sigdia(self.ctx, a.ctypes.data_as(C.c_void_p), n, C.byref(n)))
        return a

    # -- tile decomposition ---------------------------------------------------------------
    def rccl_init(self, id128, rank, nranks):
        buf = (C.c_char * 128).from_buffer_copy(bytes(id128))
        self._chk(self.lib.blomgpu_rccl_init(self.ctx, buf, rank, nranks))

    def rccl_init_2d(self, id128, rank, npx, npy):
        buf = (C.c_char * 128).from_buffer_copy(bytes(id128))
        self._chk(self.lib.blomgpu_rccl_init_2d(self.ctx, buf, rank, npx, npy))

    def rccl_attach_barotp_global(self, glob, isizes, jsizes):
        """every rank solves the whole 2-D barotropic domain on `glob`, a BlomGpu of the global domain (blomgpu.h)"""
        a = (C.c_int * len(isizes))(*[int(x) for x in isizes])
        b = (C.c_int * len(jsizes))(*[int(x) for x in jsizes])
        self._chk(self.lib.blomgpu_rccl_attach_barotp_global(self.ctx, glob.ctx, a, b))
        self._bt_global = glob               # keep it alive as long as the tile

    def rccl_init_layout(self, id128, rank, layout):
        """join the communicator as rank `rank` of a blom_amd.tiles.TileLayout, ragged tables included
        (blomgpu_rccl_init_table; a tensor-product layout takes the path of rccl_init_2d)"""
        buf = (C.c_char * 128).from_buffer_copy(bytes(id128))
        t = [a.ctypes.data_as(C.c_void_p) for a in layout.tables()]
        self._chk(self.lib.blomgpu_rccl_init_table(self.ctx, buf, rank, layout.npx, layout.npy, *t))

    def rccl_attach_barotp_layout(self, glob, layout):
        """rccl_attach_barotp_global for a TileLayout: the windows of its non-empty tiles, in rank order"""
        t = [a.ctypes.data_as(C.c_void_p) for a in layout.tables()]
        self._chk(self.lib.blomgpu_rccl_attach_barotp_table(self.ctx, glob.ctx, layout.npx, layout.npy, *t))
        self._bt_global = glob

    def rccl_crc(self, name, lev0, nlev, itype=1):
        """xccrc of the whole decomposed domain over the RCCL ranks (a collective: every rank calls it, every rank gets the
        value); on a context without RCCL, crc()"""
        v = C.c_uint(0)
        self._chk(self.lib.blomgpu_rccl_crc(self.ctx, name.encode(), lev0, nlev, itype, C.byref(v)))
        return v.value

    def rccl_force_ns_exchange(self, on=True):
        self._chk(self.lib.blomgpu_rccl_force_ns_exchange(self.ctx, int(on)))

    def rccl_finalize(self):
        self.lib.blomgpu_rccl_finalize(self.ctx)

    def timer_reset(self):
        self._chk(self.lib.blomgpu_timer_reset(self.ctx))

    def timer_get(self, what):
        ms, n = C.c_double(0), C.c_int(0)
        self._chk(self.lib.blomgpu_timer_get(self.ctx, what.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


def rccl_unique_id():
    lib = load_library()
    buf = (C.c_char * 128)()
    if lib.blomgpu_rccl_unique_id(buf):
        raise BlomGpuError("ncclGetUniqueId failed")
    return bytes(buf)


class TileGroup:
    """Several tiles of one domain on ONE device in one process (one host thread per tile): the
    in-process halo transport used to check decomposition independence (tests)."""

    def __init__(self, npx, npy, layout=None):
        """layout: a blom_amd.tiles.TileLayout whose table the group follows (blomgpu_group_create_table) -- needed for a
        ragged one, where only the non-empty tiles are attached and run a thread"""
        self.lib = load_library()
        self.h = C.c_void_p()
        if layout is None:
            self.lib.blomgpu_group_create(npx, npy, C.byref(self.h))
        else:
            assert (layout.npx, layout.npy) == (npx, npy)
            t = [a.ctypes.data_as(C.c_void_p) for a in layout.tables()]
            if self.lib.blomgpu_group_create_table(npx, npy, layout.itdm, layout.jtdm, *t, C.byref(self.h)):
                raise BlomGpuError(self.lib.blomgpu_last_error(None).decode())
        self.npx, self.npy = npx, npy

    @classmethod
    def for_layout(cls, layout):
        return cls(layout.npx, layout.npy, layout)

    def attach(self, gpu, px, py):
        gpu._chk(self.lib.blomgpu_group_attach(self.h, gpu.ctx, px, py))

    def destroy(self):
        self.lib.blomgpu_group_destroy(self.h)
