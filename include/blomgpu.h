/* blomgpu.h -- C-ABI of the MI355X-native BLOM dynamical core (libblomgpu.so).
 *
 * BLOM has no plugin/FFI layer: its operator API is the uniform Fortran stage signature
 *     subroutine <stage>(m,n,mm,nn,k1m,k1n)           phy/mod_blom_step.F90:89-253
 * acting on module-global, halo-4 arrays a(1-nbdy:idm+nbdy, 1-nbdy:jdm+nbdy, k)
 * (phy/mod_state.F90:34-86, phy/mod_xc.F90:45).  This header is what an
 * ISO_C_BINDING shim for that path binds to (INTEGRATION.md shows the shim): one entry
 * point per stage with the reference's name and argument meaning, field upload/download
 * for the module arrays, the xctilr halo update and the xccrc-style checksum.
 *
 * Conventions
 *  - all indices are the reference's 1-based Fortran values, passed by value;
 *  - a field is addressed by the reference's variable name ("dp", "utflx", "pgfxm" ...);
 *    element (i,j,k) lives at  (i+nbdy-1) + (idm+2*nbdy)*((j+nbdy-1) + (jdm+2*nbdy)*(k-1));
 *  - every function returns 0 on success, non-zero on error (the reference prints and
 *    calls xcstop/xchalt, e.g. phy/mod_advect.F90:166-172; the Fortran shim maps a
 *    non-zero status to xchalt); blomgpu_last_error() gives the text;
 *  - no host fallback exists: without a HIP device every compute entry fails.
 */
#ifndef BLOMGPU_H
#define BLOMGPU_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct blomgpu_ctx blomgpu_ctx;

/* Tile geometry, cf. module dimensions (bld/blom_dimensions:152-265) and xcspmd
 * (phy/mod_xc.F90:1332-2027): this tile owns i0+1..i0+ii, j0+1..j0+jj of the
 * itdm x jtdm global grid.  nreg as in phy/mod_bigrid.F90:81-95. */
typedef struct {
  int idm, jdm, kdm;   /* tile extents (== ii, jj) and number of layers            */
  int nbdy;            /* halo width, must be 4 (phy/mod_xc.F90:45)                 */
  int itdm, jtdm;      /* global grid size                                          */
  int i0, j0;          /* tile offsets                                              */
  int nreg;            /* 0 closed, 1 periodic-i, 2 arctic, 3 doubly periodic, 4 periodic-j */
  int ntr;             /* number of advected tracers (trc/mod_tracers.F90:225)      */
  int device;          /* HIP device ordinal                                        */
} blomgpu_dims;

int  blomgpu_create(const blomgpu_dims *dims, blomgpu_ctx **out);
int  blomgpu_destroy(blomgpu_ctx *ctx);
const char *blomgpu_last_error(const blomgpu_ctx *ctx);   /* ctx may be NULL */

/* Namelist-type options that the reference keeps as module variables set by rdlim
 * (phy/mod_rdlim.F90:137-155): baclin, batrop, delt1, dlt, lstep, nstep, pref, mdv2hi ...
 * cb, cwbdts, cwbdls, wuv1 ... wbaro, mommth, pgfmth, advmth, bmcmth, vcoord_tag ... */
int  blomgpu_set_real(blomgpu_ctx *ctx, const char *name, double v);
int  blomgpu_set_int (blomgpu_ctx *ctx, const char *name, int v);
int  blomgpu_set_str (blomgpu_ctx *ctx, const char *name, const char *v);
int  blomgpu_get_real(blomgpu_ctx *ctx, const char *name, double *v);
/* The names the three setters know, one table (blom_amd/csrc/api.hip): index 0, 1, ... until the return value is non-zero;
 * kind 0 = blomgpu_set_real, 1 = blomgpu_set_int, 2 = blomgpu_set_int (stored as v != 0), 3 = blomgpu_set_str. */
int  blomgpu_option_name(int index, char *buf, int cap, int *kind);

/* Field access.  nlev is the size of the third dimension (trc: 2*kdm*ntr). */
int  blomgpu_field_info(blomgpu_ctx *ctx, const char *name, int *nlev, int *is_int);
int  blomgpu_upload  (blomgpu_ctx *ctx, const char *name, const void *host, int nlev);
int  blomgpu_download(blomgpu_ctx *ctx, const char *name, void *host, int nlev);
/* Integer masks ip,iu,iv,iq (phy/mod_xc.F90:62-65), built by bigrid on the host. */
int  blomgpu_set_masks(blomgpu_ctx *ctx, const int *ip, const int *iu, const int *iv,
                       const int *iq);

/* xctilr(a,l1,ld,mh,nh,itype), phy/mod_xc.F90:2342 / :4222.  `lev0` (1-based) is the
 * level of `name` that the reference passes as a(1-nbdy,1-nbdy,lev0). */
int  blomgpu_xctilr(blomgpu_ctx *ctx, const char *name, int lev0, int l1, int ld,
                    int mh, int nh, int itype);

/* CRC32 of levels lev0..lev0+nlev-1 over the tile interior where the mask of the grid selected
 * by itype (1/11 p, 2/12 q, 3/13 u, 4/14 v) is 1 -- chksum/xccrc for a single tile
 * (phy/mod_checksum.F90:41-74, phy/mod_xc.F90:4164). */
int  blomgpu_crc(blomgpu_ctx *ctx, const char *name, int lev0, int nlev, int itype, unsigned *crc);

/* xccrc on a decomposed domain (phy/mod_xc.F90:2195-2322): after the halo update the reference performs there, the
 * CRCs of the 9-column strips this tile owns (those whose centre column lies in the tile), out[row 1..jdm][strip];
 * *l0 = global index of its first strip, *ns = their number.  Chaining the strips of a tile row in global order, then
 * the rows, gives the decomposition-independent checksum (blom_amd/tiles.py: chain_crc); for one tile that is
 * blomgpu_crc. */
int  blomgpu_crc_strips(blomgpu_ctx *ctx, const char *name, int lev0, int nlev, int itype, unsigned *out, int cap,
                        int *l0, int *ns);
/* Name of registered field number `index` (0-based; 1 when there is none): enumeration for hosts that move whole states. */
int  blomgpu_field_name(blomgpu_ctx *ctx, int index, char *buf, int cap);

/* Stages: same names, same argument meaning as the reference. */
int  blomgpu_init_fluxes(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n); /* phy/mod_state.F90:341   */
int  blomgpu_tmsmt1 (blomgpu_ctx *, int nn);                                             /* phy/mod_tmsmt.F90:209   */
int  blomgpu_tmsmt2 (blomgpu_ctx *, int m, int mm, int nn, int k1m);                     /* phy/mod_tmsmt.F90:281   */
int  blomgpu_initms (blomgpu_ctx *, int mm);                                             /* phy/mod_tmsmt.F90:161   */
int  blomgpu_advect (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);     /* phy/mod_advect.F90:59   */
int  blomgpu_pbcor1 (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);     /* phy/mod_pbcor.F90:66    */
int  blomgpu_pbcor2 (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);     /* phy/mod_pbcor.F90:416   */
int  blomgpu_diffus (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);     /* phy/mod_diffus.F90:41   */
int  blomgpu_pgforc (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);     /* phy/mod_pgforc.F90:438  */
int  blomgpu_momtum (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);     /* phy/mod_momtum.F90:215  */
int  blomgpu_convec (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);      /* phy/mod_convec.F90:43   */
/* xcsum (phy/mod_xc.F90:4116): reproducible masked sum of one level of a device field (strips of 9 points per
 * row, rows added serially); itype selects the mask as for xctilr (p-grid: the mask of the global sums, ips).
 * budget_sums (phy/mod_budget.F90:95-196; active with the option cnsvdi = 1): mass weighted global sums of S, T, tracer 1, the
 * TKE tracer (itrtke >= 1) and the GLS tracer (gls, itrgls >= 1) after call `ncall` of the step, and with call 5 (isopyc_bulkml) or 4
 * (the other coordinates) the salt correction's sum sc (:182-194); the column sums are left in util1..util4 as the reference leaves
 * them.  The numbers are also filed into the record of the step the option "nstep" names (below).
 * blomgpu_budget_get(which = 0 sdp | 1 tdp | 2 trdp | 3 tkedp | 4 glsdp) (:49-57). */
int  blomgpu_xcsum(blomgpu_ctx *, const char *name, int lev, int itype, double *sum);
int  blomgpu_budget_sums(blomgpu_ctx *, int ncall, int n, int nn);
int  blomgpu_budget_get(blomgpu_ctx *, int which, int ncall, int n, double *value);
/* The rest of mod_budget.  blomgpu_budget_init (:73-93): mass0 = xcsum(pb(:,:,1)*scp2), kept in the context (blomgpu_budget_mass0).
 * blomgpu_budget_output(ctx, m) (:335-352), for a host that sequences the stages itself: the sums sf tf trf of (salflx+salrlx),
 * (surflx+surrlx) and trflx(1) times scp2*delt1 into the record of step "nstep"; the line of the step is blomgpu_budget_line's.
 *
 * blomgpu_set_int "budget_step" = 1 (with "cnsvdi" = 1): blomgpu_step runs the seven calls and budget_output's sums itself, where
 * blom_step has them (phy/mod_blom_step.F90:96-245), two launches a call and no host synchronisation; the records of a call's steps
 * come back in one copy at its end.  Such a call does not leave util1..util4 as the reference leaves them (scratch planes); with
 * use_graph = 1 a budgeted step runs as plain launches; over RCCL ranks the option is refused at the first step.
 *
 * A record is 39 doubles: [(ncall-1)*5 + which] the five sums of the seven calls, [35] sc, [36..38] sf tf trf as computed at the END of
 * that step.  The library holds the records of the last blomgpu_step call and the one of the step before it (a stage-by-stage host:
 * the last 64 steps): blomgpu_budget_steps gives the first step and the count, blomgpu_budget_record fails for any other step.
 * blomgpu_budget_line: the terms budget_output(m) writes at step nstep (:211-331; nstep - 1 is the line's first column) into file
 * 0 salbud | 1 tembud | 2 tkebud | 3 glsbud | 4 trcbud (6 terms each) | 5 trcbudtot (7 terms): calls 1..5, sc, sf, tf, trf of step
 * nstep - 1, calls 6 and 7 of step nstep, the surface flux in the 4th difference (isopyc_bulkml) or the 3rd.  It fails if step
 * nstep - 1 has no record (the reference's nstep > nstep1 + 1) or the tracer set does not call for the file: blomgpu_budget_files gives
 * the files it calls for (:231-268) as a mask, bit `file` set. */
int  blomgpu_budget_init(blomgpu_ctx *);
int  blomgpu_budget_output(blomgpu_ctx *, int m);
int  blomgpu_budget_mass0(blomgpu_ctx *, double *mass0);
int  blomgpu_budget_steps(blomgpu_ctx *, int *first_step, int *count);
int  blomgpu_budget_record(blomgpu_ctx *, int nstep, double *rec39);
int  blomgpu_budget_files(blomgpu_ctx *, int *mask);
int  blomgpu_budget_line(blomgpu_ctx *, int nstep, int file, double *terms, int *nterms);
/* exp() as the kernels evaluate it -- the algorithm and bits of the glibc libm that the reference's compiled Fortran
 * calls (blom_amd/csrc/exp_libm.h; phy/mod_barotp.F90:183,205, phy/mod_diapfl.F90:204) -- elementwise on host arrays. */
int  blomgpu_exp(blomgpu_ctx *, int n, const double *x, double *y);
/* pow() as the kernels evaluate it: likewise the algorithm and bits of glibc's pow (blom_amd/csrc/pow_libm.h; the real powers of the
 * TKE closure and of the surface layer's stability function in difest_vertical_iso, phy/mod_difest.F90:2881-2886, :3056-3058). */
int  blomgpu_pow(blomgpu_ctx *, int n, const double *x, const double *y, double *z);
/* sin() and atan2() as the kernels evaluate them: the algorithms and bits of glibc's IBM Accurate Mathematical Library routines
 * (blom_amd/csrc/sin_libm.h, atan2_libm.h; the alignment of the flow with the topography under rhsctp, phy/mod_difest.F90:2331). */
int  blomgpu_sin(blomgpu_ctx *, int n, const double *x, double *z);
int  blomgpu_atan2(blomgpu_ctx *, int n, const double *y, const double *x, double *z);
/* phy/mod_difest.F90:735 difest_isobml, the whole routine: halo updates, interface pressure, ustar3, niw_ke_tendency (blomgpu_stage
 * "difest_isobml_pre") and the diffusivity estimates difest_common_iso (:353), difest_vertical_iso (:2629), difest_lateral_iso (:2040)
 * -> difint, difiso, difdia, difwgt (and the TKE tracers' source step).  Options: blomgpu_set_real "egc", "eggam", "eglsmn", "egmndf",
 * "egmxdf", "egidfq", "ri0", "tkepf"; blomgpu_set_int "eddf2d", "edsprs", "edanis", "redi3d", "edfsmo", "edritp_opt" (1 shear, 2 large
 * scale), "edwmth_opt" (1 smooth, 2 step), "bdmtyp", "iwdflg", "bdmldp", "rhsctp" (with blomgpu_set_real "rhiscf" and the fields
 * "betatp", "hangle": since round 6), "gls" (use_GLS, the two-equation closure: since round 6).  Inputs that
 * depend on the grid only and need the host's libm are uploaded as planes: "tdmls" (tidal mixing length scale, :2926-2927) and, with
 * bdmldp, "bdmlq" = log(2 bvf0 / max(1e-9, |coriop|)) with the option "bdml_logc" = log(2 bvf0 / cori30).
 * PARITY UNPINNED: cross-checked against the reference's real module compiled against interface-only stand-ins for CVMix. */
int  blomgpu_difest_isobml(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
/* the derived constants of the TKE closure (initke, phy/mod_tke.F90:133-160) as this library evaluates them, by the reference's names */
int  blomgpu_tke_const(const char *name, double *value);
int  blomgpu_updtrc (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);      /* trc/mod_tracers_update.F90:152: its idlage_step, idlage/mod_idlage.F90:57 */
int  blomgpu_sfcstr (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);      /* phy/mod_sfcstr.F90:33 (empty for channel/fuk95/noforcing) */
int  blomgpu_diapfl (blomgpu_ctx *, int n, int nn, int k1n);                             /* phy/mod_diapfl.F90:49   */
int  blomgpu_barotp (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);     /* phy/mod_barotp.F90:148  */
/* phy/mod_eddtra.F90:1808 eddtra.  vcoord_type = 'isopyc_bulkml': eddtra_intdif_isopyc_bulkml / eddtra_gm_isopyc_bulkml (:153, :228).
 * The other coordinates: eddtra_ale (:1001) -- Gent-McWilliams below the mixed layer, tapered inside it, plus the mixed layer
 * restratification blomgpu_set_str "mlrmth" = "fox08" (default), "bod23" (Bodner et al. 2023, since round 5: ustar3 / wstar3 are
 * uploaded fields -- their producer for this coordinate is CVMix's KPP, which is not built) or "none"; blomgpu_set_real "ce", "tau_mlr", "tau_growing_hbl", "tau_decaying_hbl", "tau_growing_hml",
 * "tau_decaying_hml", "lfmin", "mlbl_max_ratio" (:53-94, same defaults).  Inputs by name: nslpx, nslpy (interfaces), difint, mld,
 * OBLdepth (mod_difest's boundary layer depth); state: hbl_tf, hml_tf1, hml_tf (the running means), hml_tfbnd.  Writes umfltd,
 * vmfltd, umflsm, vmflsm and the heat and salt components u/v{t,s}fl{td,sm}. */
int  blomgpu_eddtra (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
/* Halo updates the reference performs inside stages that are outside the hot path
 * (phy/mod_cmnfld_routines.F90:1171-1196: temp/saln halos and the kfpla halo through util1, phy/mod_difest.F90:750-772: halos + interface pressure p out to ii+3) and the
 * dp-halo/dpu/dpv tail of mxlayr (phy/mod_mxlayr.F90:1266-1310). */
/* cppm (advmth = 'cppm'): stencil tags and coefficient tables from ip, scpx, scpy; call once after the
 * grid has been uploaded.  phy/mod_cppm.F90:2504 (init_cppm, called from blom_init). */
int  blomgpu_init_cppm(blomgpu_ctx *);
int  blomgpu_halo_cmnfld2(blomgpu_ctx *, int n);
/* cmnfld2 for isopyc_bulkml (phy/mod_cmnfld_routines.F90:1158): the halo updates above plus, with eitmth = 'gm', the
 * filtered buoyancy frequency (:61-227) and the neutral slopes nslpx/nslpy, nnslpx/nnslpy (:423-652) eddtra consumes. */
int  blomgpu_cmnfld2(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
/* cmnfld1 for isopyc_bulkml (phy/mod_cmnfld_routines.F90:1090): cmnfld_z (:885-921), z and dz from phi, p, dp, temp, saln
   of time level m; called after tmsmt2 (phy/mod_blom_step.F90:233).  PARITY UNPINNED (the module needs netCDF). */
int  blomgpu_cmnfld1(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
int  blomgpu_halo_difest (blomgpu_ctx *, int nn);
int  blomgpu_mxlayr_tail (blomgpu_ctx *, int nn, int k1n);
/* phy/mod_thermf.F90:35 thermf(m,n,mm,nn,k1m,k1n), for expcnf = 'channel' channel/mod_thermf_channel.F90:56: surface fluxes of
 * heat (surflx, sswflx, surrlx), salt (salflx, brnflx, salrlx) and tracers (trflx), the friction velocity ustar, from the forcing
 * fields swa, nsf, eva, lip, sop, rnf, rfi, ustarw and the climatologies sstclm, ricclm, sssclm; options blomgpu_set_real "trxday",
 * "srxday", "trxdpt", "srxdpt", "trxlim", "srxlim", "sref", "area", "xmi", blomgpu_set_int "l1mi".."l5mi" (mod_time's position
 * in the year), "aptflx", "apsflx", "ditflx", "disflx", "srxbal" (refused when set: not built).  Its two global sums (xcsum,
 * phy/mod_xc.F90:2071) are formed in the global domain's order on decomposed domains too: "area" is the GLOBAL ocean area, and
 * RCCL ranks need the global context of the replicated barotropic solve (blomgpu_rccl_attach_barotp_global).  PARITY UNPINNED (the module
 * imports the netCDF-bound mod_ben02): cross-checked against the real module behind a stand-in, tests/test_xcheck_thermf.py. */
int  blomgpu_thermf (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
/* The surface forcing of the coupled experiment, expcnf = 'cesm' (BLOM inside NorESM; blom_amd/csrc/stage_thermf_cesm.hip).
 *
 * blomgpu_inifrc_cesm: cesm/mod_cesm.F90:175-200 inifrc_cesm -- l1ci = l2ci = 1, and idarlx's zeroing of tflxdi / sflxdi / nflxdi when
 * "ditflx" / "disflx" are set (phy/mod_idarlx.F90:89-114); the file reads stay the host's (sstclm ricclm sssclm tflxap sflxap are
 * uploaded by name).  It is also the declaration that the coupler's forcing exists: it creates the fields
 *   <x>_da (2 levels) for x = ustarw lip sop eva rnf rfi fmltfz sfl swa nsf hmlt ficem ztx mty  (cesm/mod_cesm.F90:67-97)
 *   hmlt frzpot mltpot (:61-64)   ztx mty sst_stream sss_stream ice_stream (phy/mod_forcing.F90)   thermf_util (1 + ntr planes)
 *   tflxap sflxap tflxdi sflxdi (48 levels each: allocated when their option -- "aptflx" "apsflx" "ditflx" "disflx" -- is set on a declared
 *   context or is on at the declaration, or when first named to an entry point)   ipwocn (integer)
 * Until it has been called nothing of this is allocated, launched or changed, and blomgpu_thermf / blomgpu_sfcstr refuse
 * expcnf = 'cesm' ("... is not built on the device until blomgpu_inifrc_cesm has been called").  Afterwards, with expcnf = 'cesm':
 *   blomgpu_getfrc_cesm  cesm/mod_cesm.F90:202-263 getfrc_cesm: x = w1*x_da(l1ci) + w2*x_da(l2ci) for the fourteen fields above, w1 from
 *                        "smtfrc", "nstep", "nstep_in_cpl" with the C library's cos; stage name "getfrc_cesm"
 *   blomgpu_sfcstr       cesm/mod_sfcstr_cesm.F90:33-65 sfcstr_cesm: taux = ztx, tauy = mty
 *   blomgpu_thermf       cesm/mod_thermf_cesm.F90:58-432 thermf_cesm, both vertical coordinates; reads p, dp / temp / saln at both time
 *                        levels, the tracers, the fields getfrc_cesm fills, sstclm ricclm sssclm or (blomgpu_set_int
 *                        "use_stream_relaxation") sst_stream sss_stream ice_stream, salt_corr trc_corr; writes surflx sswflx surrlx
 *                        salflx brnflx salrlx hmltfz trflx ustar frzpot mltpot, t_rs_nonloc s_rs_nonloc (hybrid coordinates), zeroes
 *                        salt_corr trc_corr; "aptflx" "apsflx" apply tflxap / sflxap, "ditflx" "disflx" add to tflxdi / sflxdi at
 *                        level ntld, "srxbal" balances the salinity relaxation over ipwocn (single tile).  Time of the year:
 *                        blomgpu_set_int "nstep", "nstep_in_day", "nday_of_year", "nday_in_year" (:74-84).  The freezing point is
 *                        the stand-alone driver's swtfrz (drivers/nocoupler/mod_swtfrz.F with phy/mod_eos.F90:133-136).
 *                        blomgpu_get_real "sflxc" returns the correction of the virtual salt flux (:342-343).
 *   blomgpu_step         runs getfrc_cesm behind init_fluxes (phy/mod_blom_step.F90:116), sfcstr in front of pgforc (:163), thermf at :188
 *                        (full_physics and the hybrid sequence).  With "use_graph" = 1 it refuses: the per-step scalars are kernel
 *                        arguments.
 * The options of this section ("smtfrc", "nstep_in_cpl", "l1ci", "l2ci", "use_stream_relaxation", "nstep_in_day", "nday_of_year") go through
 * blomgpu_set_int like every other; blomgpu_option_name does not list them (it lists the table of the options that exist without the declaration).
 * blomgpu_get_real "thermf_cesm_launches": the kernel launches thermf_cesm has issued so far (four a call up to 32 planes in the batch:
 * ntr' <= 31, 29 with srxbal; two more per further 32).
 * blomgpu_cesm_nflxdi: mod_forcing's nflxdi(48).  blomgpu_xcsum_batch: xcsum (phy/mod_xc.F90:4116) of nlev consecutive levels of a
 * field at once, through the kernels thermf_cesm's 1 + ntr + 2 sums take; mask "ips" or the name of an integer field (single tile). */
int  blomgpu_inifrc_cesm(blomgpu_ctx *);
/* one level (1-based) of a real field from one host plane: what a coupling interval uploads of a _da pair is level l2ci alone */
int  blomgpu_upload_level(blomgpu_ctx *, const char *name, const void *host, int lev);
int  blomgpu_getfrc_cesm(blomgpu_ctx *);
int  blomgpu_cesm_nflxdi(blomgpu_ctx *, int out[48]);
int  blomgpu_xcsum_batch(blomgpu_ctx *, const char *name, int lev0, int nlev, const char *mask, double *sums);
/* The surface forcing of the forced ocean-ice experiment, expcnf = 'ben02clim' / 'ben02syn' / 'single_column' (Bentsen & Drange 2002;
 * blom_amd/csrc/stage_thermf_ben02.hip): the one family in which BLOM itself carries sea ice.
 * blomgpu_inifrc_ben02: the declaration that this forcing exists.  Refused unless expcnf is one of the three, on a context that has
 *                       called blomgpu_inifrc_cesm (and the other way round), and with "use_graph" = 1.  It creates, all zero:
 *   hicem hsnwm ustari tauxice tauyice iagem                          (phy/mod_seaice.F90:35-42; ficem exists)
 *   tsrfm ticem                                                       (ben02/mod_thdysi.F90:32-33)
 *   tsi dfl albw alb rnfins rnfres, tsi_tda tml_tda sml_tda alb_tda fice_tda   (ben02/mod_ben02.F90:150-214)
 *   ztx mty, thermf_util (1 + ntr planes), ipwocn (integer), tflxap sflxap tflxdi sflxdi (48 levels; memory on first use)
 *   Until it has been called nothing of this exists and blomgpu_sfcstr / blomgpu_thermf refuse the three experiments as before.
 *   Afterwards:
 *   blomgpu_sfcstr       ben02/mod_sfcstr_ben02.F90:35-72 sfcstr_ben02: ficem, hicem with a halo of one, then
 *                        taux = ztx (1 - facice) + tauxice facice at u-points, tauy likewise at v-points
 *   blomgpu_thermf       ben02/mod_thermf_ben02.F90:65-703 thermf_ben02, both vertical coordinates: the slab ice / snow thermodynamics
 *                        with ben02/mod_thdysi.F90:60-78's parameters, lead freezing and lateral melt, the runoff reservoir
 *                        (rnfins -> rnfres -> rnf), fmltfz sfl brnflx salflx hmltfz surflx sswflx, trflx, the relaxation (sstclm in
 *                        kelvin, ricclm sssclm; "trxday" .. "srxlim", "aptflx" "apsflx" "ditflx" "disflx" "srxbal", "nstep_in_day",
 *                        "nday_of_year"), iagem, ustar; it adds to the five _tda planes and to ntda (:356-360, :671) and to nflxdi (:115).
 *                        swtfrz: drivers/nocoupler/mod_swtfrz.F with phy/mod_eos.F90:137-141's coefficients.  Four launches a call up to
 *                        32 planes in the batch (blomgpu_get_real "thermf_ben02_launches"); "srxbal" is refused on tiles.
 *   blomgpu_step         runs sfcstr in front of pgforc (phy/mod_blom_step.F90:163) and thermf at :188 (full_physics and the hybrid
 *                        sequence); there is no getfrc stage: asflux (ben02/mod_ben02.F90:1602-1918) stays the host's, which uploads
 *                        swa nsf dfl lip sop eva rfi rnfins ustarw tsi albw ztx mty ustari tauxice tauyice by name.  A call of N steps keeps
 *                        them fixed and leaves ntda = N.
 * blomgpu_ben02_ntda: mod_ben02's ntda.  blomgpu_ben02_reset_tda: the five _tda planes and ntda to zero (ben02/mod_ben02.F90:1623-1624,
 * :1701-1705: what asflux does once it has used the averages). */
int  blomgpu_inifrc_ben02(blomgpu_ctx *);
int  blomgpu_ben02_ntda(blomgpu_ctx *, int *ntda);
int  blomgpu_ben02_reset_tda(blomgpu_ctx *);
/* phy/mod_mxlayr.F90:130 mxlayr(m,n,mm,nn,k1m,k1n): the bulk mixed layer of vcoord_type = 'isopyc_bulkml' (turbulent kinetic
 * energy balance, detrainment / entrainment, surface forcing, the new layer structure at the velocity points), called after
 * thermf (phy/mod_blom_step.F90:188-192).  Reads the surface fluxes surflx, surrlx, sswflx, salflx, brnflx, salrlx, trflx, the
 * friction velocity ustar and ustar3 = ustar**3, idkedt, swfc2, swal2; options blomgpu_set_real "rm0", "rm5", "niwgf", "niwbf",
 * "ce", "tau_mlr", "lfmin", "swamxd", blomgpu_set_str "mlrttp".  PARITY UNPINNED (mod_mxlayr imports netCDF-bound modules):
 * cross-checked against the real module behind stand-ins, tests/test_xcheck_mxlayr.py. */
int  blomgpu_mxlayr (blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
/* phy/mod_ale_regrid_remap.F90:1486 ale_regrid_remap(m,n,mm,nn,k1m,k1n): regrid the layer interfaces and remap T, S, tracers, u, v
 * (vcoord_type = 'plevel' and 'cntiso_hybrid' with regrid_method 'direct' or 'nudge'); with blomgpu_set_int
 * "ltedtp_opt" = 2 (ltedtp = 'neutral', phy/mod_diffusion.F90:123-124) also the neutral diffusion of phy/mod_ndiff.F90 between
 * regridding and remapping (option "ndiff_surface_align"; reads difiso, dpml, pu, pv; adds to utflx .. vsflx, sets utflld ..,
 * nslpx, nslpy).  PARITY: cross-checked against the real modules (mod_ale_regrid_remap behind the mod_dia stand-in,
 * mod_ndiff as it is), tests/test_xcheck_ale.py.  Options: blomgpu_set_str "vcoord_type", "ale_reconstruction_method", "ale_regrid_method",
 * "ale_tracer_limiting", "ale_velocity_limiting"; blomgpu_set_int "ale_upper_bndr_ord", "ale_lower_bndr_ord", "ale_k_range_plevel",
 * "ale_dktzu", "ale_dktzl", "ale_{density,tracer,velocity}_pc_{upper,lower}_bndr"; blomgpu_set_real "ale_dpmin_interior" [m],
 * "ale_regrid_nudge_ts", "ale_stab_fac_limit", "ale_dpvar_fac", "ale_smooth_diff_max" -- the variables of &ALE_REGRID_REMAP
 * (:1193-1201) with the reference's defaults (:69-95). */
int  blomgpu_ale_regrid_remap(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
/* phy/mod_ale_vdiff.F90:50 ale_vdifft, :245 ale_vdiffm: implicit vertical diffusion of T, S, tracers (with the surface fluxes and
 * their non-local transport) and of u, v.  Inputs by name: kdiff_t, kdiff_s, kvisc_m, t_{ns,sw,rs}_nonloc, s_{nb,br,rs}_nonloc
 * (kdm+1 levels), surflx, sswflx, surrlx, salflx, brnflx, salrlx, trflx (ntr planes); salt_corr, trc_corr accumulate. */
int  blomgpu_ale_vdifft(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
/* the halo updates of difest_lateral_hybrid (which = 0, phy/mod_difest.F90:826-831) / difest_vertical_hybrid (which = 1, :877-878) */
int  blomgpu_halo_difest_hyb(blomgpu_ctx *, int which, int k1n);
/* phy/mod_cmnfld_routines.F90:352 cmnfld_bfsqi_ale (phy/mod_blom_step.F90:199): p from dp, interface buoyancy frequency */
int  blomgpu_cmnfld_bfsqi_ale(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
/* phy/mod_ale_forcing.F90:45 ale_forcing: t_sw_nonloc, s_br_nonloc, buoyfl from the surface fluxes, the absorption bands swfc1,
 * swfc2, swal1, swal2 (mod_swabs) and mld (mod_cmnfld); blomgpu_set_real "swamxd", "brine_mlbase_frac" */
int  blomgpu_ale_forcing(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
int  blomgpu_ale_vdiffm(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
/* 1-D module arrays: "plevel", the kdm pressure levels [g cm-1 s-2 as the model's p] of vcoord_type = 'plevel'
 * (phy/mod_vcoord.F90:99, :948-970) */
int  blomgpu_set_vector(blomgpu_ctx *, const char *name, const double *v, int nv);

/* Time-mean diagnostics accumulated on the device: diaacc of phy/mod_dia.F90:1092 (phy/mod_blom_step.F90:239) for the accumulators
 * that read arrays the device holds -- acch2d (:1547-1745, :5182), maxh2d (:1752, :5285), sqh2d (:1780-1786, :5409), acclyr
 * (:1793-1913, :5471) -- one output group.  A name is the reference's ACC_* suffix in lower case: "ub", "sealv", "maxbld", "uvel",
 * "temp" ... (the table: blom_amd/csrc/stage_diaacc.hip, enumerated by blomgpu_dia_name; what is left out: DESIGN.md 7).
 * Writing files and the scaling by 1/nacc (wrth2d, wrtlyr, wrtlvl) stay on the host.  The z-level (Levitus) interpolation does
 * not: a layer is mapped onto the depth levels with THAT step's interfaces (diazlv :4737-4993, acclvl :5709-5781), so the level
 * names below are accumulated on the device every step like the others.
 *
 * blomgpu_dia_select: `names` is a blank-separated list that REPLACES the selection; "" deselects everything and frees the
 *   accumulators.  Adds diaini's dependencies (:598-608: a dp-weighted name selects "dp", "uvel" selects "dpu", "vvel" "dpv"),
 *   allocates one array [slot][level][padded plane], initialises it as inih2d / inilyr do (:5001-5113: inival*mask over the whole
 *   padded plane; inival = -1e33 for "maxbld", 0 otherwise) and sets nacc = 0.  An unknown name, or "tke" / "gls_psi" without
 *   itrtke >= 1 / gls (:1907), fails with a message that names it and leaves the previous selection and its contents in force.
 * blomgpu_diaacc: the stage (also blomgpu_stage "diaacc"): nacc = nacc + 1 (:1123-1125), then the accumulation at the owned points
 *   of each accumulator's grid.  Without a selection it does nothing.  With one, blomgpu_step runs it at the end of every step
 *   (after cmnfld1); "sealv", "slvsq", "dz" read cmnfld1's z / dz, and a step whose sequence does not run cmnfld1 refuses them.
 * blomgpu_dia_nacc: the number of accumulated steps (nacc_phy).
 * blomgpu_dia_get: the accumulator's padded plane (2-D names) or kdm planes (layer names), laid out as blomgpu_download's.
 * blomgpu_dia_finalize: finlyr (:6114-6185) in place for the weighted layer pairs of :2597-2611 -- acc/wgt where wgt > 1e-11, else
 *   nf90_fill_double = 9.9692099683868690e+36.  (finh2d, :6054: the table has no weighted 2-D row.)
 * blomgpu_dia_reset: inifld (:5864) for the selection: re-initialises and sets nacc = 0.
 * blomgpu_dia_name: row `index` of the table (0, 1, ... until the return value is non-zero); is_lyr 0 = 2-D, 1 = kdm layers,
 *   2 = ddm depth levels; grid 0 p, 1 u, 2 v.  Rows 0..77 are the 2-D and layer rows, rows 78..110 the depth-level rows.
 *
 * Depth-level names (33; isopycnic coordinate :2000-2053, :2119-2168, :2222-2271): "uvellvl" and the u-fluxes "uflxlvl utflxlvl
 *   usflxlvl umfltdlvl umflsmlvl utfltdlvl utflsmlvl utflldlvl usfltdlvl usflsmlvl usflldlvl", the same twelve on v, and on p
 *   "salnlvl templvl bfsqlvl difintlvl difisolvl difdialvl tkelvl gls_psilvl dzlvl".  They add no dependencies; "tkelvl" /
 *   "gls_psilvl" need what "tke" / "gls_psi" need; "dzlvl" reads cmnfld1's dz like "dz".  Under cntiso_hybrid / plevel the
 *   reference forms "uvellvl vvellvl salnlvl templvl" inside ale_regrid_remap (:1944, :2059, :2174 leave them out): see
 *   blomgpu_dia_alarm below; until the alarm has been declared those four are refused there.  blomgpu_dia_get returns ddm planes for a level name; blomgpu_dia_finalize applies msklvl (:6659-6738) to
 *   them: at every owned point the levels whose upper bound is not above the bottom become nf90_fill_double.  Not built:
 *   accilv (difvmolvl difvholvl difvsolvl), pvlvl, the tracer levels (:3688-3788).
 * blomgpu_dia_set_levels: the depth levels as bnds[ddm][2] = (upper, lower) bound of each level in metres, increasing and
 *   contiguous (bnds[d][1] == bnds[d+1][0]), ddm <= 128; otherwise, or while a level name is selected, it fails with a message and
 *   changes nothing.  bnds == NULL with ddm == 0 restores the default, the 35 levels of :111-128.
 * blomgpu_dia_levels_levitus2x: the 70 levels of LEVITUS2X (:130-159); refused while a level name is selected.
 * blomgpu_dia_get_levels: *ddm, and the first min(cap, ddm) rows of the bounds into bnds (may be NULL).
 *
 * "templvl salnlvl uvellvl vvellvl" under cntiso_hybrid / plevel: not diazlv's weights but a REMAP of that step's vertical
 *   reconstructions (PLM / PPM / PQM, the ALE options) onto the depth levels, a second prepare_remapping + remap with n_dst = ddm
 *   (phy/mod_ale_regrid_remap.F90:1059-1151 remap_trc_diazlv_jslice; u :1817-1853, v :1913-1949).  Target edges of a column:
 *   p_dst(1) = p_src(1), p_dst(kd) = min(depthslev_bnds(1,kd)/bath, 1)*(p_src(kk+1) - p_src(1)) + p_src(1), p_dst(ddm+1) = p_src(kk+1),
 *   bath = pbath | ubath | vbath.  acc = acc + rm(kd) for T and S, acc = acc + rm(kd) + ub | vb for u | v, at the owned wet points.
 *   A step takes ONE sample, and which one depends on the reference's output alarm alarm_phy:
 *     - while the alarm the previous step's diaout_alarms left is 0, ale_regrid_remap takes it (:1524-1531): time level n at the
 *       START of the step, from the reconstructions the layer remap uses, plus ub | vb (n);
 *     - when this step's alarm is 1, ale_remap_diazlv takes it (:2014-2017, phy/mod_blom_step.F90:271-273): time level m at the END
 *       of the step, reconstructed afresh, plus ub | vb (m).
 *   So a window of N steps holds N - 1 start-of-step samples and one end-of-step sample; the step after an output takes none at its
 *   start.  The library cannot know the output schedule: the host declares it.
 * blomgpu_dia_alarm: alarm_phy(1) of the one output group, 0 or 1 (anything else is refused); it holds until set again.  A fresh
 *   context is UNDECLARED, and while it is, the four names stay refused under cntiso_hybrid / plevel at blomgpu_dia_select and at
 *   blomgpu_step (without a declared alarm the sums would not be the reference's).  With alarm 0 the stage ale_regrid_remap (inside
 *   blomgpu_step and through blomgpu_stage) accumulates the selected ones of the four; with alarm 1 it does not.  blomgpu_step never
 *   changes the alarm.  A change drops captured step graphs (option "use_graph"), as a selection does.  Under isopyc_bulkml the
 *   alarm is ignored: the four names are diaacc's (k_dialvl) as before.
 * blomgpu_ale_remap_diazlv: phy/mod_ale_regrid_remap.F90:1986-2201 with its arguments (also blomgpu_stage "ale_remap_diazlv").
 *   Accumulates the selected ones of the four names when the alarm is 1; does nothing when it is 0 or undeclared or none is
 *   selected; refused under isopyc_bulkml.  The host calls it where blom_step does: after blomgpu_step has returned, with the
 *   indices of that last step, before blomgpu_dia_finalize.  blomgpu_step never calls it.  The reference's window of N steps:
 *     blomgpu_dia_alarm(1); step(1); blomgpu_dia_alarm(0); step(N-1); blomgpu_dia_alarm(1); blomgpu_ale_remap_diazlv(..); finalize
 *   nacc counts as before (diaacc, once per step); blomgpu_dia_finalize's msklvl and blomgpu_dia_reset treat the four like every
 *   level row.  Not built: the idlage level (:1132-1146).
 *
 * Density-class names (6, kind 3; :1368-1538): the mass fluxes binned into the diagnostic density classes sigdia with THAT step's
 *   interface densities and a search index carried down the column -- "umfll umfltdl umflsml" on u (acclyr :1457, :1461, :1465;
 *   sources uflx, umfltd, umflsm at k + nn) and "vmfll vmfltdl vmflsml" on v (:1530, :1534, :1538; vflx, vmfltd, vmflsm).  kdm
 *   planes each, unweighted: they add no dependencies (diaini :627-658 adds none), blomgpu_dia_get returns kdm planes and
 *   blomgpu_dia_finalize leaves them as they are (finlyr's list :2597-2611 does not hold them).  A class name needs a sigdia table
 *   and is refused without one; it is refused under vcoord_type = 'plevel', where nothing writes sigint.  Under isopyc_bulkml the
 *   stage writes sigint at the owned p-points (:1372-1390), under cntiso_hybrid it takes the sigint ale_regrid_remap left; both
 *   exchange its one-point halo (:1392).  blomgpu_dia_name does NOT enumerate these rows:
 * blomgpu_dia_name_all: the whole table -- the 111 rows of blomgpu_dia_name in their order, then the six class rows with kind 3.
 * blomgpu_dia_set_sigdia: the kdm class densities (n == kdm; the reference's sigdia, taken as given as mod_vcoord.F90:978-1005
 *   does).  NULL with n == 0 clears the table.  A wrong n, a non-finite value, or a call while a class name is selected fails with
 *   a message and changes nothing.
 * blomgpu_dia_get_sigdia: *n (0: no table), and the first min(cap, n) values into out (may be NULL).
 *
 * Vertical mass flux (diavfl, :4633-4733, called at :2279): "wflx wflx2" (kdm layers, p-grid, unweighted) and "wflxlvl wflx2lvl"
 *   (ddm depth levels, p-grid) -- the flux through the layer interfaces, carried from the bottom up out of THAT step's uflx, vflx
 *   and dp - dpold, the same on the depth levels out of the step's increments of uflxlvl / vflxlvl, and the squares of both.  The
 *   four are one group (diaini :615-618, :644-647, :673-680): any of them selects all four, "uflx vflx uflxlvl vflxlvl", and two
 *   internal ddm-level slots "uflxold" (u) and "vflxold" (v) (ACC_UFLXOLD / ACC_VFLXOLD, :1921-1942) that hold last step's uflxlvl /
 *   vflxlvl.  blomgpu_dia_select refuses the two internal names; blomgpu_dia_get hands them out while the group is selected.  The
 *   group uses and freezes the level table like every level name, and is admitted under every vertical coordinate.  Each step the
 *   stage exchanges the one-point halo of uflxlvl and vflxlvl (xctilr, halo_uv / halo_vv, :4681-4684; on the arctic patch the
 *   sign flips across the seam and the second half of row jj of vflxlvl is the seam's mirror, as the reference's).  While the
 *   group is selected blomgpu_step keeps tmsmt1 a launch of its own (the option tmsmt_ahead has no effect): diavfl needs the
 *   dpold of the previous step.  blomgpu_dia_finalize applies msklvl to "wflxlvl wflx2lvl" (:2676-2677) and leaves "wflx wflx2"
 *   alone.  Neither blomgpu_dia_name nor blomgpu_dia_name_all enumerates these rows:
 * blomgpu_dia_name_full: the whole table -- the 117 rows of blomgpu_dia_name_all in their order, then "wflx wflx2" (kind 1),
 *   "wflxlvl wflx2lvl" (kind 2), "uflxold vflxold" (kind 4: ddm depth levels, internal -- not selectable by name).
 *
 * Column-derived names (10; all on the p-grid, owned masked points): what diaacc derives from THAT step's water column before it
 *   accumulates it -- a search or a nonlinear function of the column, so no time mean of the state gives it.
 *   "sbot tbot" (2-D; :1251-1294, acch2d :1697, :1700): salinity and temperature averaged over the lowest dpbot = onem (:196) of the
 *     column; where that is thinner than onemm, the values of layer 1.
 *   "t20d t17d" (2-D; :1296-1366, acch2d :1712, :1715): depth of the 20 and 17 degC isotherms -- 0. where the first layer thicker
 *     than onecm is colder, z(kk+1) where no layer thicker than onecm is, the interpolation between two layer centres otherwise.
 *   "mldl82 mldl82mn mldl82mx mldl82sq" (2-D; acch2d :1706, minh2d :1755 / :5347-5405, maxh2d :1758, sqh2d :1773): the mixed layer
 *     depth after Levitus (1982), phy/mod_cmnfld_routines.F90:933-995, its minimum (initial value +1e33*mask, :5900), maximum
 *     (-1e33*mask, :5901) and square.  The field is cmnfld1's: under cntiso_hybrid / plevel it is the mixed layer depth cmnfld1
 *     forms anyway, under isopyc_bulkml cmnfld1 forms it while one of the four is selected (:1109-1113), writing mldl82 only.
 *   "t20d t17d" and the four mldl82 names read z / dz: under isopyc_bulkml a step sequence that does not run cmnfld1 (options
 *     cmnfld1 = 0 and full_physics = 0) refuses them at blomgpu_dia_select and again at blomgpu_step.  A host that drives the
 *     stages itself calls blomgpu_cmnfld1 in front of blomgpu_diaacc (phy/mod_blom_step.F90:233-239) and sets cmnfld1 = 1.
 *   "avdsg dpvor" (kdm layers, unweighted; :1203-1247): absolute vorticity at the four corners of the p-point, masked and summed,
 *     times the layer's potential density difference, and the thickness momtum used for the vorticity (mod_momtum.F90:477-496)
 *     summed likewise.  Either name selects both (diaini :681-682).  blomgpu_dia_finalize divides "avdsg" by "dpvor" where dpvor >
 *     1e-11, else nf90_fill_double (finlyr(ACC_AVDSG, ACC_DPVOR, 'p'), :2608), and leaves "dpvor" alone.
 *   blomgpu_dia_name, _name_all and _name_full do NOT enumerate these rows:
 * blomgpu_dia_name_ext: the whole table -- the 123 rows of blomgpu_dia_name_full in their order, then "sbot tbot t20d t17d mldl82
 *   mldl82mn mldl82mx mldl82sq" (kind 0) and "avdsg dpvor" (kind 1): 133 rows.  Not built: mldb04 and its kin, pvlvl. */
int  blomgpu_dia_select(blomgpu_ctx *, const char *names);
int  blomgpu_diaacc(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
int  blomgpu_dia_nacc(blomgpu_ctx *, int *nacc);
int  blomgpu_dia_get(blomgpu_ctx *, const char *name, double *out);
int  blomgpu_dia_finalize(blomgpu_ctx *);
int  blomgpu_dia_reset(blomgpu_ctx *);
int  blomgpu_dia_name(int index, char *buf, int cap, int *is_lyr, int *grid);
int  blomgpu_dia_set_levels(blomgpu_ctx *, const double *bnds /* [ddm][2] */, int ddm);
int  blomgpu_dia_levels_levitus2x(blomgpu_ctx *);
int  blomgpu_dia_get_levels(blomgpu_ctx *, double *bnds /* [cap][2] */, int cap, int *ddm);
int  blomgpu_dia_name_all(int index, char *buf, int cap, int *kind, int *grid);
int  blomgpu_dia_set_sigdia(blomgpu_ctx *, const double *sigdia, int n);
int  blomgpu_dia_get_sigdia(blomgpu_ctx *, double *out, int cap, int *n);
int  blomgpu_dia_name_full(int index, char *buf, int cap, int *kind, int *grid);
int  blomgpu_dia_name_ext(int index, char *buf, int cap, int *kind, int *grid);
int  blomgpu_dia_alarm(blomgpu_ctx *, int alarm);
int  blomgpu_ale_remap_diazlv(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);

/* What diaout_iogrp forms from the accumulators at output time (phy/mod_dia.F90:2366-2588), on the device
 * (blom_amd/csrc/stage_diaout.hip): diamer (:4004-4629), diasec (:3814-4001), the global sums and means (:2427-2588).  One output group,
 * a context that holds the whole domain.
 *
 * The 23 "msc" names have no accumulator of their own; blomgpu_dia_select takes them and selects their sources as diaini does (:557,
 *   :559, :598-670):
 *     "mmflxl mmftdl mmfsml"       overturning stream function in density space   umfll vmfll | umfltdl vmfltdl | umflsml vmflsml
 *                                  (class names: they need a sigdia table)
 *     "mmflxd mmftdd mmfsmd"       the same in depth space                         uflxlvl vflxlvl | umfltdlvl vmfltdlvl | umflsmlvl vmflsmlvl
 *     "mhflx mhftd mhfsm mhfld"    meridional heat transports                      utflx vtflx | utfltd vtfltd | utflsm vtflsm | utflld vtflld
 *     "msflx msftd msfsm msfld"    meridional salt transports                      the same on s
 *     "masstr heattr salttr"       transports through named sections               uflxlvl vflxlvl | utflxlvl vtflxlvl | usflxlvl vsflxlvl
 *     "massgs salnga tempga"       global mass, mean salinity and temperature      dp (+ saln | temp)
 *     "volgs"  "sssga sstga"       global volume; mean surface S and T             dz;  sss | sst
 * blomgpu_dia_name_msc: the 133 rows of blomgpu_dia_name_ext in their order, then these 23 with kind 5.  The earlier enumerators do
 *   not list them.
 * blomgpu_dia_set_mertra: what diamer reads from mer_orfile and mer_mifile (:4026-4108), as the caller's tables: lmax sections with
 *   latitude mtlat[l] and nind[l] points each, pts[sum nind][4] = (i, j, uflg, vflg) with i, j 1-based in the global domain; the ocean
 *   region flags oflg[jtdm][itdm]; ocn_nreg; mer_nreg meridional regions with nflg[m] flags regflg[m][20] (regflg[m][0] == 0: all ocean
 *   regions, :4242) and latitude bounds minlat[m], maxlat[m].  A point whose oflg <= 0 is dropped (:4070).  Refused with a message: an
 *   index outside 1..itdm | 1..jtdm (:4076-4086), oflg > ocn_nreg, a region flag outside 0..ocn_nreg (0 as the first flag only),
 *   lmax > itdm+jtdm and a section that keeps more than itdm+jtdm points (ldm, sdm :163-164), ocn_nreg or mer_nreg outside 1..32.
 *   NULL tables with lmax == 0 clear the table.
 * blomgpu_dia_set_sections: what diasec reads from sec_sifile (:3838-3866): sec_num sections of nsi[s] points, pts[sum nsi][4] =
 *   (i, j, usi, vsi); equat_sec the 1-based section that takes the upper-350 m sums (:3849), -1 for none.  With equat_sec >= 1 the
 *   depth levels must be the 35-level table (k350 = 12, w350 = 1., :112-113) or LEVITUS2X (25, .5, :131-132): a table of
 *   blomgpu_dia_set_levels is refused, here and again at blomgpu_dia_reduce.  NULL tables with sec_num == 0 clear the table.
 *   Both tables are copied to the device once, may be set at any time, and are read by blomgpu_dia_reduce only.
 * blomgpu_dia_reduce: runs what the selection asks for on the context's stream, the results into a small device buffer; the host is
 *   not made to wait.  Where diaout_iogrp has these computations: after the last blomgpu_step of the window (and after
 *   blomgpu_ale_remap_diazlv where that applies), before blomgpu_dia_finalize -- which writes fill values into the level rows, so
 *   from finalize until blomgpu_dia_reset or a new selection a reduce is refused.  Also refused, each with its reason: nacc == 0,
 *   an msc name whose table has not been set, no msc name selected, sssga | sstga with "area" <= 0, a context that is a tile of a group
 *   or an RCCL rank.  It reads accumulators only: twice gives the same bytes, no accumulator and no model field changes.
 *   The bits are the reference's: r = (.5*spcifh | .5*g2kg | .5)/((grav*baclin)*real(nacc)); the running sums of :4188-4212, :4340-4371,
 *   :4492-4559, :3903-3953 at the wet u | v points and 0. elsewhere; the section sums serial in the table's order, mflx_or(l,o) =
 *   (mflx_or(l,o) + real(uflg)*ucum) + real(vflg)*vcum, one per ocean region; the region sums of :4235-4256; nf90_fill_double where
 *   mtlat lies outside the region's bounds, for the eight transports where the region has no point (:4254), in depth space below
 *   kmax(l,m) (:4449-4467); the global numbers with xcsum's order, salnga and tempga divided by the unscaled massgs.
 *   Options (blomgpu_set_int; blomgpu_option_name does not list them): "diaout_entries" (1..256, default 256) section points per
 *   pass and "diaout_levels" (1..8, default 8) levels per chunk of the section kernel; the results do not depend on them.
 * blomgpu_dia_msc_get: the result of one selected name from the last reduce into out[cap], its shape into dims[3] -- the reference's
 *   (:4113-4119): [mer_nreg][kdm | ddm][lmax] for the stream functions, [mer_nreg][lmax][1] for the transports, [sec_num][1][1] for the
 *   section transports, [1][1][1] for the global names.  cap == 0 asks for the shape alone (out may be NULL).  Refused before a
 *   reduce, for a name that is not selected, and with a cap that is neither 0 nor enough (dims is filled all the same).
 * Not built: the barotropic stream function btmstr (:2376-2424), tiles and RCCL ranks, several output groups. */
int  blomgpu_dia_name_msc(int index, char *buf, int cap, int *kind, int *grid);
int  blomgpu_dia_set_mertra(blomgpu_ctx *, int lmax, const double *mtlat, const int *nind, const int *pts /* [sum nind][4] */,
                            const int *oflg /* [jtdm][itdm] */, int ocn_nreg, int mer_nreg, const int *nflg,
                            const int *regflg /* [mer_nreg][20] */, const double *minlat, const double *maxlat);
int  blomgpu_dia_set_sections(blomgpu_ctx *, int sec_num, const int *nsi, const int *pts /* [sum nsi][4] */, int equat_sec);
int  blomgpu_dia_reduce(blomgpu_ctx *);
int  blomgpu_dia_msc_get(blomgpu_ctx *, const char *name, double *out, int cap, int *dims /* [3] */);

/* The end of blom_step (phy/mod_blom_step.F90:96-252).  Everything here is off until an option declares it; an undeclared context steps
 * as before.  The options are set like every other (blomgpu_set_int / _real / _str); blomgpu_option_name does not list them.
 *
 * "step_time" = 1: blomgpu_step does step_time (phy/mod_time.F90:182-219) on the host in front of every step.  With ns1 the incremented
 *   step number, sd = "nstep_in_day" and nd = "nday_in_year": where ns1 % sd == 0 the day moves on, nday_of_year = nday_of_year % nd + 1;
 *   then xmi = (nday_of_year - 1 + (ns1 % sd)/double(sd))*12./double(nd), l3mi = int(xmi) + 1, xmi = xmi - (l3mi - 1), and l1mi l2mi
 *   l4mi l5mi the months around l3mi -- in double, in the reference's order, written where the setters write "nday_of_year", "xmi",
 *   "l1mi" .. "l5mi".  The day rule equals date_offset + set_day_of_year inside a year and across a year's end whose successor has the
 *   same length: a host on a leap calendar ends its call at the year's last step and sets "nday_in_year" in between.  Refused with
 *   nstep_in_day < 1 or nday_in_year < 1.  One blomgpu_step of nstep_in_cpl steps then equals that many steps of the reference.
 * blomgpu_iniswa: iniswa (phy/mod_swabs.F90:216-609) for the method "swamth" names -- "top-layer" and "jerlov" ("jwtype" 1..5) fill swfc1
 *   swfc2 swal1 swal2 at the owned wet p-points; "spatial_frac_attlen" leaves the four planes to the host's uploads; "chlorophyll_ma94"
 *   and "chlorophyll_ohl03" ("chlopt" = "climatology") create the fields "chl10c" (12 levels: log10 of the monthly chlorophyll
 *   concentration, halos included, uploaded by name) and "chl10", and the second builds Ohlmann's four 401-entry tables.  Another word,
 *   a jwtype outside 1..5 and another chlopt are refused in the reference's words.
 * blomgpu_updswa: updswa (:611-732) -- chl10 interpolated in time from chl10c with l1mi..l5mi and xmi, clamped to [-2, 1], then the
 *   four planes from Morel and Antoine's polynomials or Ohlmann's table; returns at once for the other methods.  blomgpu_step runs it
 *   behind getfrc (phy/mod_blom_step.F90:122) while a chlorophyll method is declared.
 * blomgpu_fwbbal: fwbbal (phy/mod_forcing.F90:361-441).  "sprfac" = 1 creates and zeroes the fields "eiacc" and "pracc" (restart
 *   variables: up and down by name) and sets "prfac" = 1 (inivar_forcing, :345-357); it creates "ipwocn" where the context has none
 *   and expects an upload.  Each call accumulates eva + fmltfz and lip + sop + rnf + rfi times baclin; when nday_of_year == 1 and
 *   nstep % nstep_in_day == 0 it weights both with scp2, sums them under ipwocn in xcsum's order, sets prfac = -prfac*totei/totpr
 *   (blomgpu_get_real "prfac") and zeroes both.  blomgpu_step runs it behind diaacc (:242) while sprfac is set.
 * blomgpu_chkvar: chkvar (phy/mod_chkvar.F90:77-141) with "chkvar" = 1 -- NaN (a /= a) or Inf (a*0 /= 0) in dp, temp or saln of time
 *   level n at an owned wet p-point fails the call with the reference's line and global indices, "blom: chkvar: dp is NaN at (i =   7,
 *   j =  12, k =   3)": of several hits the one the serial reference meets first (j, then k, then i, then dp NaN, dp Inf, temp NaN,
 *   temp Inf, saln NaN, saln Inf).  blomgpu_step runs it last in every step (:252) and reads its words back every "check_period" steps.
 * "use_graph" = 1 beside any of the four is refused: their per-step scalars are kernel arguments. */
int  blomgpu_iniswa(blomgpu_ctx *);
int  blomgpu_updswa(blomgpu_ctx *);
int  blomgpu_fwbbal(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);
int  blomgpu_chkvar(blomgpu_ctx *, int m, int n, int mm, int nn, int k1m, int k1n);

/* Generic dispatcher over the entries above ("advect", "tmsmt1", ...). */
int  blomgpu_stage(blomgpu_ctx *, const char *stage, int m, int n, int mm, int nn,
                   int k1m, int k1n);

/* Device-resident time stepping: `nsteps` passes of the stage sequence of
 * phy/mod_blom_step.F90:96-253 (hot-path stages only), starting from step count
 * `nstep` (value before step_time).  Returns the new step count in *nstep.
 * Option "use_graph" = 1 (default 0: replay measures 2 % slower than plain launches on ROCm 7.2): on a single tile the
 * sequence is captured in the third step after the last change of an option or of the time step (the fourth step from rest) -- for both parities of the time levels at once -- and
 * replayed as HIP graphs from then on (steps with the stage timers on, "timing" = 1, run plain launches beside the graphs);
 * blomgpu_get_real "graph_steps" / "graph_failures" count the replays / the captures that failed.
 *
 * The heat and salt flux diagnostics -- utflx usflx vtflx vsflx, utfltd usfltd vtfltd vsfltd, utflld usflld vtflld vsflld -- hold
 * what the reference holds, on both time levels, when the call has returned.  Inside a call of more than two steps they are
 * kept current only while something reads them every step (a diaacc selection with one of them as a source, "csdiag", a
 * captured graph, the hybrid coordinates): nothing in a step reads them, and the steps that could leave nothing visible in them
 * skip the passes over memory that only keep them up to date.  A call that fails part-way leaves them undefined.
 * blomgpu_get_real "flux_diag_steps_skipped" counts the steps that skipped since the context was created;
 * blomgpu_keep_flux_diagnostics(ctx, 1) keeps the arrays current in every step (0, the default, gives the above back). */
int  blomgpu_step(blomgpu_ctx *, int *nstep, int nsteps);
int  blomgpu_keep_flux_diagnostics(blomgpu_ctx *, int on);

/* Tile decomposition (xcspmd/xctilr, phy/mod_xc.F90:1332-3188).  A context is one tile
 * (dims.i0/j0/itdm/jtdm).  Two transports serve blomgpu_xctilr and every halo update inside the stages:
 *  - RCCL: one process per GPU, tiles laid out along i; rank 0 creates the 128-byte id, the launcher
 *    distributes it, every rank calls blomgpu_rccl_init;
 *  - an in-process group (several tiles on one device, one host thread per tile) used by the parity tests. */
int  blomgpu_rccl_unique_id(void *id128);
int  blomgpu_rccl_init(blomgpu_ctx *, const void *id128, int rank, int nranks);          /* npx = nranks, npy = 1 */
int  blomgpu_rccl_init_2d(blomgpu_ctx *, const void *id128, int rank, int npx, int npy);  /* rank = px + npx*py */
int  blomgpu_rccl_force_ns_exchange(blomgpu_ctx *, int on);   /* test hook, see comm_rccl.hip */
/* The barotropic solve (barotp, phy/mod_barotp.F90:330-1003: 2.5 lstep substeps per step, one xctilr per substep pair in
 * the reference) replicated on every rank instead of decomposed: `global` is a second context on the same device that
 * spans the whole itdm x jtdm domain (kdm >= 3, the global masks and grid metrics uploaded); isizes[npx] / jsizes[npy]
 * are the widths / heights of the tile columns / rows.  From then on blomgpu_barotp of the tile gathers the 2-D fields
 * the solver reads (one grouped exchange), solves on `global`, and takes its window of the results. */
int  blomgpu_rccl_attach_barotp_global(blomgpu_ctx *tile, blomgpu_ctx *global, const int *isizes, const int *jsizes);
/* xccrc of the whole decomposed domain (phy/mod_xc.F90:2195-2322, chksum phy/mod_checksum.F90:41-74) over the RCCL ranks: a
 * collective -- every rank calls it with the same arguments and every rank gets the same value, the single tile's checksum of
 * the whole itdm x jtdm domain.  Each tile's strips (blomgpu_crc_strips) travel to rank 0, which chains them in global order and
 * sends the result back.  On a context without RCCL it is blomgpu_crc. */
int  blomgpu_rccl_crc(blomgpu_ctx *, const char *name, int lev0, int nlev, int itype, unsigned *crc);
int  blomgpu_rccl_finalize(blomgpu_ctx *);
typedef struct TileGroup blomgpu_group;
int  blomgpu_group_create(int npx, int npy, blomgpu_group **out);
/* Ragged tile layouts: the general table of xcspmd (phy/mod_xc.F90:1332-1720) as the reference's patch.input files give it --
 * every tile row with its own cut, tiles shrunk to their sea points, all-land tiles eliminated.  i0_pe[npy*npx], ii_pe[npy*npx]
 * (m fastest; 0-based first column minus one as i0_pe(m,n), ii_pe = 0: eliminated), j0_pe[npy], jj_pe[npy].  Ranks number the
 * non-empty tiles only, m fastest, then n (:1545-1560).  The entries above are the tensor-product special case and keep their
 * paths: a tensor-product table given here is passed on to them.  What a ragged table changes in xctilr:
 *  - E-W (:1726-1745, :3131-3178): the neighbour is the previous / next non-empty tile of the row, and only if it touches this
 *    one; otherwise the halo is vland.  A row wraps periodically only if it starts at 0 and ends at itdm (:1591-1594).
 *  - N-S (:1747-1990, :3036-3106): a tile's columns are covered by several tiles of the row below / above, one segment each;
 *    columns over no tile are vland.  With the arctic patch (nreg = 2) the top row consists of equal tiles (:1480-1506);
 *    eliminated twin tiles there are refused by the RCCL transport.
 *  - xcsum / xccrc: the 9-column strips are anchored in global columns; a tile without a touching neighbour also owns the
 *    strips centred within nbdy columns beyond that edge (:1686-1710).
 * Both transports apply the same rule point for point.  blomgpu_group_create_table needs the domain's itdm, jtdm (no context
 * exists yet); the others take them from the context. */
int  blomgpu_rccl_init_table(blomgpu_ctx *, const void *id128, int rank, int npx, int npy, const int *i0_pe, const int *ii_pe,
                             const int *j0_pe, const int *jj_pe);
int  blomgpu_rccl_attach_barotp_table(blomgpu_ctx *tile, blomgpu_ctx *global, int npx, int npy, const int *i0_pe,
                                      const int *ii_pe, const int *j0_pe, const int *jj_pe);
int  blomgpu_group_create_table(int npx, int npy, int itdm, int jtdm, const int *i0_pe, const int *ii_pe, const int *j0_pe,
                                const int *jj_pe, blomgpu_group **out);
int  blomgpu_group_attach(blomgpu_group *, blomgpu_ctx *, int px, int py);
int  blomgpu_group_destroy(blomgpu_group *);

/* Synchronise the context's stream (all entries above are asynchronous on it). */
int  blomgpu_sync(blomgpu_ctx *);

/* Timing of the dominant kernel with HIP events on the context's stream: average
 * duration [ms] of kernel class `what` ("remap", "momtum", ...) since the last reset. */
int  blomgpu_timer_reset(blomgpu_ctx *);
int  blomgpu_timer_get(blomgpu_ctx *, const char *what, double *ms_total, int *launches);

#ifdef __cplusplus
}
#endif
#endif
