"""sfcstr_ben02 and thermf_ben02 restated in numpy, operator for operator, in float64: ben02/mod_sfcstr_ben02.F90:44-61 and
ben02/mod_thermf_ben02.F90:96-671 with the parameters of ben02/mod_thdysi.F90:60-78 and ben02/mod_ben02.F90:119, :216, phy/mod_intp1d.F90,
the stand-alone driver's swtfrz with the coefficients inieos sets for these experiments (phy/mod_eos.F90:137-141) and xcsum in the
reference's strip and row order (tests/thermf_cesm_ref.py, whose helpers this file uses: the two routines share that text).

A state is a dict {field name: array (nlev, nj, ni)} of whole padded arrays as BlomGpu.get returns them; the routines change the arrays
they write in place, at the owned wet points only.  Every branch of the reference is a np.where over both sides, evaluated everywhere
(numpy does not contract; max / min are `a > b ? a : b` / `a < b ? a : b` as amdflang lowers them).  exp and **.28 come from the C
library, element by element (math.exp, math.pow).  `seen` counts the points that take each branch: the tests assert on it."""
import math

import numpy as np

from thermf_cesm_ref import (ALPHA0, EPSILT, G2KG, GLS_CMU0, GLS_M, GLS_N, GLS_P, KG2G, NBDY, ONEM, SPCIFH, T0DEG, VONKAR, ZOS, fmax, fmin,
                             intp1d, owned, rs_walk, time_of_year, xcsum)

ATF, BTF, CTF = -0.0547, 0.0, 0.0                # phy/mod_eos.F90:137-141
# ben02/mod_thdysi.F90:60-78
ALBI_F, ALBI_M, ALBS_F, ALBS_M, RHOICE, RHOSNW, RKICE, RKSNW, FUSI, FUSS = 0.70, 0.60, 0.85, 0.75, 906.0, 330.0, 2.04, 0.31, 3.02e8, 1.10e8
FICE_MAX, TICE_M, TSNW_M, HICE_NHMN, HICE_SHMN, SAGETS, SICE, CWI, CUC = 0.995, 273.05, 273.15, 0.50, 0.30, 2.0e-7, 6.0, 0.006, 1.0e3
RHOWAT, NRFETS = 1024.0, 7                       # ben02/mod_ben02.F90:216, :119
TDA = "tsi_tda tml_tda sml_tda alb_tda fice_tda".split()


def swtfrz(p, s):
    return ATF * s + BTF + CTF * p


def per_element(fn, x, sel):
    """fn of the C library at the points of sel, nan elsewhere"""
    out = np.full(x.shape, np.nan)
    out[sel] = [fn(float(v)) for v in x[sel]]
    return out


def sfcstr(s, masks, idm, jdm, nreg, halo=None):
    """sfcstr_ben02.  halo(a): the caller's xctilr of one plane with a halo of one (None: the planes come with their halos)"""
    sel = owned(masks, idm, jdm)
    fice, hice = s["ficem"][0], s["hicem"][0]
    if halo is not None:
        fice, hice = halo(fice), halo(hice)
        s["ficem"][0], s["hicem"][0] = fice, hice
    fac = (fice[:, 1:] + fice[:, :-1]) * fmin(2.0, hice[:, 1:] + hice[:, :-1]) * 0.25
    new = s["ztx"][0][:, 1:] * (1.0 - fac) + s["tauxice"][0][:, 1:] * fac
    s["taux"][0][:, 1:][sel["u"][:, 1:]] = new[sel["u"][:, 1:]]
    fac = (fice[1:] + fice[:-1]) * fmin(2.0, hice[1:] + hice[:-1]) * 0.25
    new = s["mty"][0][1:] * (1.0 - fac) + s["tauyice"][0][1:] * fac
    s["tauy"][0][1:][sel["v"][1:]] = new[sel["v"][1:]]


def thermf(s, o, idx, masks, idm, jdm, seen=None):
    """thermf_ben02(m,n,mm,nn,k1m,k1n).  o: trxday srxday trxdpt srxdpt trxlim srxlim xmi sref area baclin lmi (five months), aptflx apsflx
    ditflx disflx srxbal hybrid itrtke itrgls gls nstep nstep_in_day nday_of_year nday_in_year nreg kdm ntr.
    Returns dict(sflxc, sums: {name: value}, ntld, util: the planes summed, passive)."""
    seen = seen if seen is not None else {}
    m, n, mm, nn, k1m, k1n = idx
    kk, ntr = int(o["kdm"]), int(o["ntr"])
    sel = owned(masks, idm, jdm)["p"]
    ip = np.asarray(masks["ip"]).reshape(sel.shape)
    y, (m1, m2, m3, m4, m5) = time_of_year(o)
    ntld = m3
    dt = float(o["baclin"])
    cpsw = SPCIFH
    rnf_fac = dt / float(NRFETS * 86400)
    sag_fac = math.exp(-SAGETS * dt)
    dp, temp, saln, p = s["dp"], s["temp"], s["saln"], s["p"]
    kn = k1n - 1
    put = lambda nm, v, lev=0: s[nm][lev].__setitem__(sel, np.broadcast_to(v, sel.shape)[sel])
    cnt = lambda nm, w: seen.__setitem__(nm, seen.get(nm, 0) + int((sel & w).sum()))
    with np.errstate(all="ignore"):
        dpotl = dp[kn]
        hotl = dpotl / ONEM
        totl = temp[kn] + T0DEG
        sotl = saln[kn]
        fice, hice, hsnw, tsrf = s["ficem"][0].copy(), s["hicem"][0].copy(), s["hsnwm"][0].copy(), s["tsrfm"][0].copy()
        fice0, hice0, hsnw0 = fice, hice, hsnw
        tice_f = swtfrz(p[0], sotl) + T0DEG
        north = s["plat"][0] > 0.0
        hice_min = np.where(north, HICE_NHMN, HICE_SHMN)
        swa, nsf, albw, dfl, tsi, sop = s["swa"][0], s["nsf"][0], s["albw"][0], s["dfl"][0], s["tsi"][0], s["sop"][0]
        noice = fice * hice < 1.0e-5
        slab = ~noice
        # ---- the ice slab, :184-293, evaluated everywhere ----
        snow = fice * hsnw > 1.0e-3
        albi_h = 0.065 + 0.44 * per_element(lambda v: math.pow(v, 0.28) if v >= 0.0 else float("nan"), hice, sel & slab & ~snow)
        warm_s, warm_i = tsrf > TSNW_M - 0.1, tsrf > TICE_M - 0.1
        albi = np.where(snow, np.where(warm_s, ALBS_M, ALBS_F), np.where(warm_i, fmin(ALBI_M, albi_h), fmin(ALBI_F, albi_h)))
        tsmlt = np.where(snow, TSNW_M, TICE_M)
        cnt("noice", noice), cnt("slab", slab)
        cnt("snow_melting", slab & snow & warm_s), cnt("snow_frozen", slab & snow & ~warm_s)
        cnt("thin_melting", slab & ~snow & warm_i), cnt("thin_frozen", slab & ~snow & ~warm_i)
        cnt("albi_m_kept", slab & ~snow & warm_i & (ALBI_M < albi_h)), cnt("albi_m_cut", slab & ~snow & warm_i & ~(ALBI_M < albi_h))
        cnt("albi_f_kept", slab & ~snow & ~warm_i & (ALBI_F < albi_h)), cnt("albi_f_cut", slab & ~snow & ~warm_i & ~(ALBI_F < albi_h))
        alb_s = albi * fice + albw * (1.0 - fice)
        qswi = swa * (1.0 - albi) / (1.0 - alb_s)
        qsww_s = swa * (1.0 - albw) / (1.0 - alb_s)
        dh = sop * dt / RHOSNW
        hsnw_s = hsnw + dh
        qsnwf = dh * FUSS / dt
        fcond = RKICE * RKSNW / (RKSNW * hice + RKICE * hsnw_s)
        deg = np.abs(fcond - dfl * (2.0 - fice)) < 1.0e-3
        cnt("fcond_degenerate", slab & deg), cnt("fcond_regular", slab & ~deg)
        tsrf_s = np.where(deg, tice_f + (qswi + nsf) / fcond,
                          (qswi + nsf - dfl * (tsi + (1.0 - fice) * totl) + fcond * tice_f) / (fcond - dfl * (2.0 - fice)))
        cold = fmin(tsrf_s, tsmlt)
        qnsw_s = np.where(deg, nsf, nsf + dfl * fice * (totl - cold))
        qdamp = np.where(deg, 0.0, dfl * (cold - tsi))
        melt = tsrf_s > tsmlt
        cnt("surface_melt", slab & melt), cnt("surface_frozen", slab & ~melt)
        tsrf_s = np.where(melt, tsmlt, tsrf_s)
        qsmlt = np.where(melt, qswi + nsf + dfl * ((1.0 - fice) * (tsrf_s - totl) + tsrf_s - tsi) + fcond * (tice_f - tsrf_s), 0.0)
        tice_s = tice_f - fcond * (tice_f - tsrf_s) * hice / RKICE
        ustari = s["ustari"][0]
        qo2i = RHOWAT * cpsw * CWI * fmax(ustari, 0.2e-2) * fmin(tice_f - totl, 0.0) + CUC * fmax(tice_f - totl, 0.0)
        qbot = -fcond * (tice_f - tsrf_s) - qo2i - qdamp + qsnwf
        dh = -qsmlt * dt / FUSS
        gone = hsnw_s + dh < 0.0
        cnt("snow_exhausted", slab & gone), cnt("snow_left", slab & ~gone)
        qsmlt = np.where(gone, qsmlt - hsnw_s * FUSS / dt, 0.0)
        hsnw_s = np.where(gone, 0.0, hsnw_s + dh)
        arg = hice - (qbot + qsmlt) * dt / FUSI
        cnt("hice_clipped", slab & (0.0 > arg)), cnt("hice_kept", slab & ~(0.0 > arg))
        hice_s = fmax(0.0, arg)
        hice_s = hice_s + hsnw_s * (1.0 - sag_fac) * RHOSNW / RHOICE
        hsnw_s = hsnw_s * sag_fac
        dh = (hsnw_s * RHOSNW - hice_s * (RHOWAT - RHOICE)) / RHOWAT
        flood = dh > 0.0
        cnt("flooding", slab & flood), cnt("no_flooding", slab & ~flood)
        hice_s = np.where(flood, hice_s + dh, hice_s)
        hsnw_s = np.where(flood, hsnw_s - dh * RHOICE / RHOSNW, hsnw_s)
        # ---- :154-176 against the slab ----
        zero = np.zeros(sel.shape)
        fice = np.where(noice, zero, fice)
        hice = np.where(noice, zero, hice_s)
        hsnw = np.where(noice, zero, hsnw_s)
        alb = np.where(noice, albw, alb_s)
        qsww = np.where(noice, swa, qsww_s)
        qnsw = np.where(noice, nsf, qnsw_s)
        tsrf = np.where(noice, totl, tsrf_s)
        tice = np.where(noice, totl, tice_s)
        # ---- the open water fraction, :303-340 ----
        swfac = 1.0 - s["swfc2"][0] * per_element(math.exp, -hotl / s["swal2"][0], sel)
        heat = swfac * qsww + qnsw
        dtml = heat * 2.0 * dt / (cpsw * RHOWAT * hotl)
        frz = totl + dtml < tice_f
        q = 0.5 * (tice_f - totl) * cpsw * RHOWAT * hotl / dt
        volice = -(qsww + qnsw - q) * (1.0 - fice) * dt / FUSI
        vol = frz & (volice > EPSILT)
        df = volice / hice_min
        capped = FICE_MAX < fice + df
        fnew = fmin(FICE_MAX, fice + df)
        for hemi, w in (("nh", north), ("sh", ~north)):
            cnt("freeze_capped_" + hemi, vol & capped & w), cnt("freeze_free_" + hemi, vol & ~capped & w)
        cnt("freeze_no_volume", frz & ~vol)
        lat = ~frz & (heat > 0.0)
        fice_l = fice - heat * fice * dt / fmax(hice * FUSI + hsnw * FUSS, EPSILT)
        away = lat & (fice_l < 0.0)
        cnt("lateral_all", away), cnt("lateral_some", lat & ~away & (fice > 0.0)), cnt("neither", ~frz & ~lat)
        hice = np.where(vol, (hice * fice + volice) / fnew, np.where(away, zero, hice))
        hsnw = np.where(vol, hsnw * fice / fnew, np.where(away, zero, hsnw))
        fice = np.where(vol, fnew, np.where(lat, np.where(away, zero, fice_l), fice))
        # ---- stores and accumulations, :346-360 ----
        for nm, v in (("ficem", fice), ("hicem", hice), ("hsnwm", hsnw), ("tsrfm", tsrf), ("ticem", tice), ("alb", alb)):
            put(nm, v)
        for nm, v in (("alb_tda", alb), ("tml_tda", totl), ("sml_tda", sotl), ("fice_tda", fice), ("tsi_tda", tsrf)):
            put(nm, s[nm][0] + v)
        # ---- fluxes, :367-416 ----
        dvi = hice * fice - hice0 * fice0
        dvs = hsnw * fice - hsnw0 * fice0
        rnfres = s["rnfres"][0] + s["rnfins"][0]
        rnf = rnfres * rnf_fac
        put("rnf", rnf)
        put("rnfres", rnfres * (1.0 - rnf_fac))
        fmltfz = -(dvi * RHOICE + dvs * RHOSNW) / dt
        put("fmltfz", fmltfz)
        fwflx = s["eva"][0] + s["lip"][0] + sop + rnf + s["rfi"][0] + fmltfz
        sfl = -SICE * dvi * RHOICE / dt * G2KG
        put("sfl", sfl)
        brn_arg = -sotl * fmltfz * G2KG + sfl
        brnflx = fmax(0.0, brn_arg)
        cnt("brnflx_clipped", 0.0 > brn_arg), cnt("brnflx_pos", brnflx > 0.0)
        vrtsfl = -sotl * fwflx * G2KG
        scp2 = s["scp2"][0]
        util = [-(float(o["sref"]) * fwflx * G2KG + vrtsfl + s["salt_corr"][0] * G2KG / (2.0 * dt)) * scp2]
        put("salt_corr", 0.0)
        hmltfz = (dvi * FUSI + dvs * FUSS) / dt
        put("hmltfz", hmltfz)
        put("surflx", -(swa + nsf + hmltfz))
        put("sswflx", -qsww * (1.0 - fice0))
        # ---- tracers, :423-451 ----
        itrtke, itrgls, gls = int(o.get("itrtke", -1)), int(o.get("itrgls", -1)), int(o.get("gls", 0))
        passive = []
        for nt in range(1, ntr + 1):
            if itrtke >= 1 and nt == itrtke:
                put("trflx", 0.0, nt - 1)
                continue
            if itrtke >= 1 and nt == itrgls:
                if gls:
                    tke = s["trc"][(itrtke - 1) * 2 * kk + kn]
                    pw = np.zeros(sel.shape)
                    pw[sel] = [math.pow(v, GLS_M) for v in tke[sel]]
                    put("trflx", -GLS_N * s["difdia"][0] * (GLS_CMU0 ** GLS_P) * pw * (VONKAR ** GLS_N) * ZOS ** (GLS_N - 1.0), nt - 1)
                else:
                    put("trflx", 0.0, nt - 1)
                continue
            tf = -s["trc"][(nt - 1) * 2 * kk + kn] * fwflx
            put("trflx", tf, nt - 1)
            util.append(-(tf + s["trc_corr"][nt - 1] / (2.0 * dt)) * scp2)
            put("trc_corr", 0.0, nt - 1)
            passive.append(nt)
        # ---- relaxation, :458-578 ----
        hybrid = bool(o.get("hybrid"))
        l = [int(v) - 1 for v in o["lmi"]]
        xmi = float(o["xmi"])
        clm = lambda nm: intp1d(s[nm][l[0]], s[nm][l[1]], s[nm][l[2]], s[nm][l[3]], s[nm][l[4]], xmi)
        if hybrid and (o["trxday"] > EPSILT or o["srxday"] > EPSILT):
            pbot = p[0]
            for k in range(kk):
                pbot = pbot + dp[k + nn]
        surrlx, trxflx = np.zeros(sel.shape), np.zeros(sel.shape)
        if o["trxday"] > EPSILT:
            sstc, rice = clm("sstclm"), clm("ricclm")
            cnt("sstc_above", sstc > tice_f), cnt("sstc_below", ~(sstc > tice_f))
            sstc = (1.0 - rice) * fmax(sstc, tice_f) + rice * tice_f
            if not hybrid:
                dpmxl = dp[nn] + dp[1 + nn]
                hmxl = dpmxl / ONEM
                tmxl = (temp[nn] * dp[nn] + temp[1 + nn] * dp[1 + nn]) / dpmxl + T0DEG
                trxflx = SPCIFH * fmin(hmxl, o["trxdpt"]) / (o["trxday"] * 86400.0) * fmin(o["trxlim"], fmax(-o["trxlim"], sstc - tmxl)) / ALPHA0
            else:
                dprsi = 1.0 / fmin(o["trxdpt"] * ONEM, pbot - p[0])
                tmxl = rs_walk(dp[nn:nn + kk], temp[nn:nn + kk], s["t_rs_nonloc"], dprsi, kk, sel, True, seen.setdefault("t_exits", {}))
                trxflx = SPCIFH * o["trxdpt"] / (o["trxday"] * 86400.0) * fmin(o["trxlim"], fmax(-o["trxlim"], sstc - tmxl)) / ALPHA0
            d = sstc - tmxl
            cnt("trxlim_hi", d > o["trxlim"]), cnt("trxlim_lo", d < -o["trxlim"])
            surrlx = -trxflx
        if o.get("aptflx"):
            a = s["tflxap"]
            surrlx = surrlx - intp1d(a[m1 - 1], a[m2 - 1], a[m3 - 1], a[m4 - 1], a[m5 - 1], y)
        put("surrlx", surrlx)
        if o.get("ditflx"):
            put("tflxdi", s["tflxdi"][ntld - 1] + trxflx, ntld - 1)
        salrlx, srxflx = np.zeros(sel.shape), np.zeros(sel.shape)
        if o["srxday"] > EPSILT:
            sssc = clm("sssclm")
            if not hybrid:
                dpmxl = dp[nn] + dp[1 + nn]
                hmxl = dpmxl / ONEM
                smxl = (saln[nn] * dp[nn] + saln[1 + nn] * dp[1 + nn]) / dpmxl
                srxflx = fmin(hmxl, o["srxdpt"]) / (o["srxday"] * 86400.0) * fmin(o["srxlim"], fmax(-o["srxlim"], sssc - smxl)) / ALPHA0
            else:
                dprsi = 1.0 / fmin(o["srxdpt"] * ONEM, pbot - p[0])
                smxl = rs_walk(dp[nn:nn + kk], saln[nn:nn + kk], s["s_rs_nonloc"], dprsi, kk, sel, False, seen.setdefault("s_exits", {}))
                srxflx = o["srxdpt"] / (o["srxday"] * 86400.0) * fmin(o["srxlim"], fmax(-o["srxlim"], sssc - smxl)) / ALPHA0
            d = sssc - smxl
            cnt("srxlim_hi", d > o["srxlim"]), cnt("srxlim_lo", d < -o["srxlim"])
            salrlx = -srxflx
            put("util2", fmax(0.0, salrlx) * scp2)
            put("util3", fmin(0.0, salrlx) * scp2)
        if o.get("apsflx"):
            a = s["sflxap"]
            salrlx = salrlx - intp1d(a[m1 - 1], a[m2 - 1], a[m3 - 1], a[m4 - 1], a[m5 - 1], y)
        put("salrlx", salrlx)
        if o.get("disflx"):
            put("sflxdi", s["sflxdi"][ntld - 1] + srxflx, ntld - 1)
        # ---- age of the ice, friction velocity, :584-594 ----
        young = fice * hice < 1.0e-5
        cnt("iage_zero", young), cnt("iage_aged", ~young)
        put("iagem", np.where(young, 0.0, (s["iagem"][0] + dt / 86400.0) * (1.0 - fmax(0.0, dvi) / (fice * hice))))
        put("ustar", fmin(ustari, 0.8e-2) * fice0 + s["ustarw"][0] * (1.0 - fice0))
        # ---- the sums and what follows from them, :608-665 ----
        seam = int(o.get("nreg", 0)) == 2
        area = float(o["area"])
        sums = dict(salt=xcsum(util[0], ip, idm, jdm, seam))
        sflxc = sums["salt"] / area
        put("salflx", -(vrtsfl + sflxc + sfl) * KG2G)
        put("brnflx", -brnflx * KG2G)
        if o["srxday"] > EPSILT and o.get("srxbal"):
            ipw = s["ipwocn"][0]
            totsrp, totsrn = xcsum(s["util2"][0], ipw, idm, jdm), xcsum(s["util3"][0], ipw, idm, jdm)
            sums.update(totsrp=totsrp, totsrn=totsrn)
            if abs(totsrp - totsrn) > 0.0:
                qp = 2.0 * totsrn / (totsrn - totsrp)
                qn = 2.0 * totsrp / (totsrp - totsrn)
                seen["qp"], seen["qn"] = qp, qn
                cur = s["salrlx"][0]
                w = sel & (ipw == 1)
                s["salrlx"][0][w] = (qp * fmax(0.0, cur) + qn * fmin(0.0, cur))[w]
        for q_, nt in enumerate(passive):
            sums["trc%d" % nt] = xcsum(util[1 + q_], ip, idm, jdm, seam)
            trflxc = sums["trc%d" % nt] / area
            put("trflx", -(s["trflx"][nt - 1] + trflxc), nt - 1)
    planes = np.zeros((len(util),) + sel.shape)
    for q_, u in enumerate(util):
        planes[q_][sel] = u[sel]
    return dict(sflxc=sflxc, sums=sums, ntld=ntld, util=planes, passive=passive)


# the branches an input set has to reach (tests/golden/make_thermf_ben02_golden.py and the tests assert every count > 0)
BRANCHES = ("noice slab snow_melting snow_frozen thin_melting thin_frozen albi_m_kept albi_m_cut albi_f_kept albi_f_cut fcond_degenerate "
            "fcond_regular surface_melt surface_frozen snow_exhausted snow_left hice_clipped hice_kept flooding no_flooding freeze_capped_nh "
            "freeze_capped_sh freeze_free_nh freeze_free_sh freeze_no_volume lateral_all lateral_some neither brnflx_clipped brnflx_pos "
            "iage_zero iage_aged").split()
RELAX_BRANCHES = "sstc_above sstc_below trxlim_hi trxlim_lo srxlim_hi srxlim_lo".split()


def missing(seen, relax=True):
    return [b for b in BRANCHES + (RELAX_BRANCHES if relax else []) if not seen.get(b, 0) > 0]
