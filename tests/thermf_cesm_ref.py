"""getfrc_cesm, sfcstr_cesm and thermf_cesm restated in numpy, operator for operator, in float64:
cesm/mod_cesm.F90:213-262, cesm/mod_sfcstr_cesm.F90:43-55, cesm/mod_thermf_cesm.F90:74-410 with phy/mod_intp1d.F90:29-52, the stand-alone
driver's swtfrz (drivers/nocoupler/mod_swtfrz.F with the coefficients inieos sets for 'cesm', phy/mod_eos.F90:133-136) and xcsum
(phy/mod_xc.F90:4116-4161) in the reference's strip and row order.

A state is a dict {field name: array (nlev, nj, ni)} of whole padded arrays as BlomGpu.get returns them; the routines change the
arrays they write in place, at the owned wet points only (do j = 1,jj; do l = 1,isp(j); do i = max(1,ifp(j,l)),min(ii,ilp(j,l))).
Every expression keeps the reference's order of operations (numpy does not contract); max / min are `a > b ? a : b` / `a < b ? a : b`
as amdflang lowers them; loops stand where numpy's own summation order would differ (xcsum, the column walks).  `seen` collects what
the tests assert about their inputs."""
import math

import numpy as np

GRAV, SPCIFH, T0DEG, ALPHA0, EPSILT, ONEM, G2KG, KG2G, PI = 9.806, 3990.0, 273.15, 1.0e-3, 1.0e-11, 9806.0, 1.0e-3, 1.0e3, 3.1415926536
ATF, BTF, CTF = 0.0, -1.8, 0.0                   # phy/mod_eos.F90:133-136
GLS_CMU0, GLS_P, GLS_M, GLS_N, VONKAR, ZOS = 0.527, 3.0, 1.5, -1.0, 0.4, 0.0002      # phy/mod_tke.F90:36-58
NBDY = 4
DA = "ustarw lip sop eva rnf rfi fmltfz sfl swa nsf hmlt ficem".split()


def fmax(a, b):
    return np.where(a > b, a, b)


def fmin(a, b):
    return np.where(a < b, a, b)


def swtfrz(p, s):
    return ATF * s + BTF + CTF * p


def intp1d(d1, d2, d3, d4, d5, x):
    a1, a2, a3 = -3.0 / 7.0, -15.0 / 7.0, 3.0 / 2.0
    b1, b2, b3, b4, b5 = 4.0 / 7.0, -16.0 / 7.0, 15.0 / 7.0, -5.0 / 7.0, 2.0 / 7.0
    c1, c2 = -1.0 / 7.0, 9.0 / 14
    a = a1 * (d1 + d5) + a2 * d3 + a3 * (d2 + d4)
    b = b1 * d1 + b2 * d2 + b3 * d3 + b4 * d4 + b5 * d5
    c = c1 * (d1 + d4) + c2 * (d2 + d3)
    return (a * x + b) * x + c


def owned(masks, idm, jdm):
    """{grid: the points the reference's loops visit}"""
    nj, ni = jdm + 2 * NBDY, idm + 2 * NBDY
    own = np.zeros((nj, ni), bool)
    own[NBDY:NBDY + jdm, NBDY:NBDY + idm] = True
    return {g: own & (np.asarray(masks["i" + g]).reshape(nj, ni) > 0) for g in "puv"}


def xcsum(a, mask, idm, jdm, skip_seam=False):
    """phy/mod_xc.F90:4116-4161 on one tile: strips of 2*nbdy+1 along a row, the strip sums added to the row sum in order, the row
    sums added serially.  mask: 2-D integers, points equal to 1 count; skip_seam: ips (the last row of an arctic patch is left out)"""
    w = 2 * NBDY + 1
    a = np.asarray(a, dtype=np.float64)[NBDY:NBDY + jdm, NBDY:NBDY + idm]
    m = (np.asarray(mask)[NBDY:NBDY + jdm, NBDY:NBDY + idm] == 1)
    if skip_seam:
        m = m.copy()
        m[jdm - 1, :] = False
    rows = np.zeros(jdm)
    for i1 in range(0, idm, w):
        strip = np.zeros(jdm)
        for i in range(i1, min(i1 + w, idm)):
            strip = np.where(m[:, i], strip + a[:, i], strip)
        rows = rows + strip
    s = rows[0]
    for j in range(1, jdm):
        s = s + rows[j]
    return float(s)


def weights(o):
    """w1, w2 of cesm/mod_cesm.F90:213-219"""
    if o.get("smtfrc"):
        ncpl = int(o["nstep_in_cpl"])
        w1 = 0.5 * (1.0 + math.cos(((int(o["nstep"]) - 1) % ncpl + 1) * PI / ncpl))
    else:
        w1 = 0.0
    return w1, 1.0 - w1


def getfrc(s, o, sel):
    w1, w2 = weights(o)
    l1, l2 = int(o.get("l1ci", 1)) - 1, int(o.get("l2ci", 1)) - 1
    for nm, g in [(nm, "p") for nm in DA] + [("ztx", "u"), ("mty", "v")]:
        da = s[nm + "_da"]
        s[nm][0][sel[g]] = (w1 * da[l1] + w2 * da[l2])[sel[g]]


def sfcstr(s, sel):
    s["taux"][0][sel["u"]] = s["ztx"][0][sel["u"]]
    s["tauy"][0][sel["v"]] = s["mty"][0][sel["v"]]


def time_of_year(o):
    """y, m1..m5 of :74-81 (1-based levels)"""
    y = (int(o["nday_of_year"]) - 1 + (int(o["nstep"]) % int(o["nstep_in_day"])) / float(o["nstep_in_day"])) * 48.0 / float(o["nday_in_year"])
    m3 = int(y) + 1
    y = y - float(m3 - 1)
    return y, ((m3 + 45) % 48 + 1, (m3 + 46) % 48 + 1, m3, m3 % 48 + 1, (m3 + 1) % 48 + 1)


def rs_walk(dp, x, frac, dprsi, kk, sel, add_t0deg, exits):
    """:224-239 / :285-300 over all columns at once, level by level: returns the mean; frac (kk+1 planes) is written at `sel`;
    exits[k] counts the columns that leave at level k (1-based), exits[0] those that never do"""
    cur = np.ones(dprsi.shape)
    mean = np.zeros(dprsi.shape)
    out = np.zeros(dprsi.shape, bool)
    where = np.zeros(dprsi.shape, np.int64)
    frac[0][sel] = 1.0
    for k in range(kk):
        nxt = cur - dp[k] * dprsi
        neg = ~out & (nxt < 0.0)
        leave = mean + x[k] * cur
        if add_t0deg:
            leave = leave + T0DEG
        mean = np.where(out, mean, np.where(neg, leave, mean + x[k] * (cur - nxt)))
        where[neg] = k + 1
        out = out | neg
        cur = np.where(out, 0.0, nxt)                  # (the tail the reference zeroes, from the exit level on)
        frac[k + 1][sel] = cur[sel]
    for k in range(kk + 1):
        exits[k] = exits.get(k, 0) + int((sel & (where == k)).sum())
    return mean


def thermf(s, o, idx, masks, idm, jdm, seen=None):
    """thermf_cesm(m,n,mm,nn,k1m,k1n).  o: trxday srxday trxdpt srxdpt trxlim srxlim xmi sref area baclin lmi (five months), aptflx apsflx
    ditflx disflx srxbal use_stream_relaxation hybrid itrtke itrgls gls nstep nstep_in_day nday_of_year nday_in_year nreg kdm ntr.
    Returns dict(sflxc, sums: {name: value}, ntld, util: the planes summed)."""
    seen = seen if seen is not None else {}
    m, n, mm, nn, k1m, k1n = idx
    kk, ntr = int(o["kdm"]), int(o["ntr"])
    sel = owned(masks, idm, jdm)["p"]
    ip = np.asarray(masks["ip"]).reshape(sel.shape)
    y, (m1, m2, m3, m4, m5) = time_of_year(o)
    ntld = m3
    baclin = float(o["baclin"])
    dp, temp, saln, p = s["dp"], s["temp"], s["saln"], s["p"]
    km, kn = k1m - 1, k1n - 1
    put = lambda nm, v, lev=0: s[nm][lev].__setitem__(sel, np.broadcast_to(v, sel.shape)[sel])
    with np.errstate(all="ignore"):
        tfrz = swtfrz(p[0], saln[kn])
        tfrzm = swtfrz(p[0], 0.5 * (saln[km] + saln[kn]))
        dpotl = dp[kn]
        totl = temp[kn] + T0DEG
        sotl = saln[kn]
        tice_f = tfrz + T0DEG
        fmltfz, sfl = s["fmltfz"][0], s["sfl"][0]
        fwflx = s["eva"][0] + s["lip"][0] + s["sop"][0] + s["rnf"][0] + s["rfi"][0] + fmltfz
        brn_arg = -sotl * fmltfz * G2KG + sfl
        brnflx = fmax(0.0, brn_arg)
        vrtsfl = -sotl * fwflx * G2KG
        scp2 = s["scp2"][0]
        util = [-(float(o["sref"]) * fwflx * G2KG + vrtsfl + s["salt_corr"][0] * G2KG / (2.0 * baclin)) * scp2]
        put("salt_corr", 0.0)
        frz_arg = tice_f - totl
        frzpot = fmax(0.0, frz_arg) * SPCIFH * dpotl / (2.0 * GRAV)
        mlt_arg = tfrzm - 0.5 * (temp[km] + temp[kn])
        mltpot = fmin(0.0, mlt_arg) * SPCIFH * 0.5 * (dp[km] + dp[kn]) / GRAV
        hmltfz = s["hmlt"][0] + frzpot / baclin
        swa = s["swa"][0]
        put("frzpot", frzpot)
        put("mltpot", mltpot)
        put("hmltfz", hmltfz)
        put("surflx", -(swa + s["nsf"][0] + hmltfz))
        put("sswflx", -swa)
        seen["frzpot_pos"] = int((sel & (frzpot > 0.0)).sum())
        seen["frzpot_zero"] = int((sel & (frzpot == 0.0)).sum())
        seen["mltpot_neg"] = int((sel & (mltpot < 0.0)).sum())
        seen["brnflx_clipped"] = int((sel & (0.0 > brn_arg)).sum())
        seen["brnflx_pos"] = int((sel & (brnflx > 0.0)).sum())
        # tracers, :165-186, and their planes, :391-393
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
            util.append(-(tf + s["trc_corr"][nt - 1] / (2.0 * baclin)) * scp2)
            put("trc_corr", 0.0, nt - 1)
            passive.append(nt)
        # relaxation, :193-322
        hybrid = bool(o.get("hybrid"))
        stream = bool(o.get("use_stream_relaxation"))
        l = [int(v) - 1 for v in o["lmi"]]
        xmi = float(o["xmi"])
        clm = lambda nm: intp1d(s[nm][l[0]], s[nm][l[1]], s[nm][l[2]], s[nm][l[3]], s[nm][l[4]], xmi)
        if hybrid and (o["trxday"] > EPSILT or o["srxday"] > EPSILT):
            pbot = p[0]
            for k in range(kk):
                pbot = pbot + dp[k + nn]
        surrlx, trxflx = np.zeros(sel.shape), np.zeros(sel.shape)
        if o["trxday"] > EPSILT:
            if stream:
                sstc, rice = s["sst_stream"][0], s["ice_stream"][0]
            else:
                sstc, rice = clm("sstclm"), clm("ricclm")
            seen["sstc_above"] = int((sel & (sstc > tice_f)).sum())
            seen["sstc_below"] = int((sel & ~(sstc > tice_f)).sum())
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
            seen["trxlim_hi"] = int((sel & (d > o["trxlim"])).sum())
            seen["trxlim_lo"] = int((sel & (d < -o["trxlim"])).sum())
            surrlx = -trxflx
        if o.get("aptflx"):
            a = s["tflxap"]
            surrlx = surrlx - intp1d(a[m1 - 1], a[m2 - 1], a[m3 - 1], a[m4 - 1], a[m5 - 1], y)
        put("surrlx", surrlx)
        if o.get("ditflx"):
            put("tflxdi", s["tflxdi"][ntld - 1] + trxflx, ntld - 1)
        salrlx, srxflx = np.zeros(sel.shape), np.zeros(sel.shape)
        if o["srxday"] > EPSILT:
            sssc = s["sss_stream"][0] if stream else clm("sssclm")
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
            seen["srxlim_hi"] = int((sel & (d > o["srxlim"])).sum())
            seen["srxlim_lo"] = int((sel & (d < -o["srxlim"])).sum())
            salrlx = -srxflx
            put("util2", fmax(0.0, salrlx) * scp2)
            put("util3", fmin(0.0, salrlx) * scp2)
        if o.get("apsflx"):
            a = s["sflxap"]
            salrlx = salrlx - intp1d(a[m1 - 1], a[m2 - 1], a[m3 - 1], a[m4 - 1], a[m5 - 1], y)
        put("salrlx", salrlx)
        if o.get("disflx"):
            put("sflxdi", s["sflxdi"][ntld - 1] + srxflx, ntld - 1)
        put("ustar", s["ustarw"][0])
        # the sums and what follows from them, :342-410
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
        for q, nt in enumerate(passive):
            sums["trc%d" % nt] = xcsum(util[1 + q], ip, idm, jdm, seam)
            trflxc = sums["trc%d" % nt] / area
            put("trflx", -(s["trflx"][nt - 1] + trflxc), nt - 1)
    planes = np.zeros((len(util),) + sel.shape)
    for q, u in enumerate(util):
        planes[q][sel] = u[sel]
    return dict(sflxc=sflxc, sums=sums, ntld=ntld, util=planes, passive=passive)
