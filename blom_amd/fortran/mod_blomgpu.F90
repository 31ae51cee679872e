! ------------------------------------------------------------------------------
! mod_blomgpu -- Fortran host side of the MI355X-native BLOM dynamical core.
!
! Thin ISO_C_BINDING layer over include/blomgpu.h.  The stage wrappers keep the
! reference's names and argument lists (phy/mod_blom_step.F90:126-227):
!     call advect(m,n,mm,nn,k1m,k1n)      call diapfl(n,nn,k1n)
!     call tmsmt1(nn)                     call tmsmt2(m,mm,nn,k1m)  ...
! so that the stage sequence of blom_step reads exactly as in the reference.  The
! reference has no return codes (it prints and calls xchalt/xcstop, e.g.
! phy/mod_advect.F90:166-172); a non-zero C status is converted to that behaviour
! in gpu_check.
!
! One tile per process (gpu_init_tile): the tile's context, a second context of the
! whole domain for the replicated barotropic solve, the RCCL transport between the
! ranks and the checksum over all of them.  Module mod_xcspmd_gpu at the end of this
! file reads and checks the reference's tile table patch.input (xcspmd).
! ------------------------------------------------------------------------------
module mod_blomgpu

  use iso_c_binding
  implicit none
  private
  ! difest_isobml below runs the whole routine when set: public, and also set by gpu_set('difest_live', 1) -- the option that makes
  ! blomgpu_step estimate the diffusivities -- so that a host sequencing the stages itself and the device-resident loop agree
  logical, save, public :: difest_estimates = .false.

  integer, parameter, public :: nbdy = 4          ! phy/mod_xc.F90:45
  type(c_ptr), save :: ctx = c_null_ptr
  type(c_ptr), save :: gctx = c_null_ptr          ! whole domain, for the replicated barotropic solve (tiles only)
  logical, save :: on_rccl = .false.
  integer, public :: idm, jdm, kdm, ntr, nreg     ! idm, jdm: this tile's extents
  ! the tile's place in the global itdm x jtdm grid (phy/mod_xc.F90: i0, j0, mnproc counts from 1, npes ranks)
  integer, public :: itdm, jtdm, i0 = 0, j0 = 0, mnproc = 1, npes = 1

  type, bind(C) :: blomgpu_dims
    integer(c_int) :: idm, jdm, kdm, nbdy, itdm, jtdm, i0, j0, nreg, ntr, device
  end type

  interface
    integer(c_int) function blomgpu_create(dims, ctxo) bind(C, name='blomgpu_create')
      import :: blomgpu_dims, c_ptr, c_int
      type(blomgpu_dims), intent(in) :: dims
      type(c_ptr), intent(out) :: ctxo
    end function
    integer(c_int) function blomgpu_destroy(c) bind(C, name='blomgpu_destroy')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    type(c_ptr) function blomgpu_last_error(c) bind(C, name='blomgpu_last_error')
      import :: c_ptr
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_set_real(c, name, v) bind(C, name='blomgpu_set_real')
      import :: c_ptr, c_int, c_char, c_double
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      real(c_double), value :: v
    end function
    integer(c_int) function blomgpu_set_int(c, name, v) bind(C, name='blomgpu_set_int')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      integer(c_int), value :: v
    end function
    integer(c_int) function blomgpu_set_str(c, name, v) bind(C, name='blomgpu_set_str')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*), v(*)
    end function
    integer(c_int) function blomgpu_upload(c, name, host, nlev) bind(C, name='blomgpu_upload')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      type(*), intent(in) :: host(*)
      integer(c_int), value :: nlev
    end function
    integer(c_int) function blomgpu_download(c, name, host, nlev) bind(C, name='blomgpu_download')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      type(*) :: host(*)
      integer(c_int), value :: nlev
    end function
    integer(c_int) function blomgpu_dia_select(c, names) bind(C, name='blomgpu_dia_select')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: names(*)
    end function
    integer(c_int) function blomgpu_dia_get(c, name, host) bind(C, name='blomgpu_dia_get')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      type(*) :: host(*)
    end function
    integer(c_int) function blomgpu_dia_nacc(c, nacc) bind(C, name='blomgpu_dia_nacc')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
      integer(c_int), intent(out) :: nacc
    end function
    integer(c_int) function blomgpu_dia_finalize(c) bind(C, name='blomgpu_dia_finalize')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_dia_reset(c) bind(C, name='blomgpu_dia_reset')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_dia_alarm(c, alarm) bind(C, name='blomgpu_dia_alarm')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
      integer(c_int), value :: alarm
    end function
    integer(c_int) function blomgpu_upload_level(c, name, host, lev) bind(C, name='blomgpu_upload_level')
      import :: c_ptr, c_int, c_char, c_double
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      real(c_double), intent(in) :: host(*)
      integer(c_int), value :: lev
    end function
    integer(c_int) function blomgpu_inifrc_cesm(c) bind(C, name='blomgpu_inifrc_cesm')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_getfrc_cesm(c) bind(C, name='blomgpu_getfrc_cesm')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_iniswa(c) bind(C, name='blomgpu_iniswa')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_updswa(c) bind(C, name='blomgpu_updswa')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_fwbbal(c, m, n, mm, nn, k1m, k1n) bind(C, name='blomgpu_fwbbal')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
      integer(c_int), value :: m, n, mm, nn, k1m, k1n
    end function
    integer(c_int) function blomgpu_chkvar(c, m, n, mm, nn, k1m, k1n) bind(C, name='blomgpu_chkvar')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
      integer(c_int), value :: m, n, mm, nn, k1m, k1n
    end function
    integer(c_int) function blomgpu_cesm_nflxdi(c, out) bind(C, name='blomgpu_cesm_nflxdi')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
      integer(c_int), intent(out) :: out(48)
    end function
    integer(c_int) function blomgpu_inifrc_ben02(c) bind(C, name='blomgpu_inifrc_ben02')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_ben02_ntda(c, ntda) bind(C, name='blomgpu_ben02_ntda')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
      integer(c_int), intent(out) :: ntda
    end function
    integer(c_int) function blomgpu_ben02_reset_tda(c) bind(C, name='blomgpu_ben02_reset_tda')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_dia_name_ext(index, buf, cap, kind, grid) bind(C, name='blomgpu_dia_name_ext')
      import :: c_int, c_char
      integer(c_int), value :: index, cap
      character(kind=c_char), intent(out) :: buf(*)
      integer(c_int), intent(out) :: kind, grid
    end function
    integer(c_int) function blomgpu_dia_set_levels(c, bnds, ddm) bind(C, name='blomgpu_dia_set_levels')
      import :: c_ptr, c_int
      type(c_ptr), value :: c, bnds
      integer(c_int), value :: ddm
    end function
    integer(c_int) function blomgpu_dia_levels_levitus2x(c) bind(C, name='blomgpu_dia_levels_levitus2x')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_dia_get_levels(c, bnds, cap, ddm) bind(C, name='blomgpu_dia_get_levels')
      import :: c_ptr, c_int
      type(c_ptr), value :: c, bnds
      integer(c_int), value :: cap
      integer(c_int), intent(out) :: ddm
    end function
    integer(c_int) function blomgpu_dia_set_sigdia(c, sigdia, n) bind(C, name='blomgpu_dia_set_sigdia')
      import :: c_ptr, c_int
      type(c_ptr), value :: c, sigdia
      integer(c_int), value :: n
    end function
    integer(c_int) function blomgpu_dia_get_sigdia(c, sigdia, cap, n) bind(C, name='blomgpu_dia_get_sigdia')
      import :: c_ptr, c_int
      type(c_ptr), value :: c, sigdia
      integer(c_int), value :: cap
      integer(c_int), intent(out) :: n
    end function
    ! diaout_iogrp's reductions (phy/mod_dia.F90:2366-2588: diamer, diasec, the global sums)
    integer(c_int) function blomgpu_dia_name_msc(index, buf, cap, kind, grid) bind(C, name='blomgpu_dia_name_msc')
      import :: c_int, c_char
      integer(c_int), value :: index, cap
      character(kind=c_char), intent(out) :: buf(*)
      integer(c_int), intent(out) :: kind, grid
    end function
    integer(c_int) function blomgpu_dia_set_mertra(c, lmax, mtlat, nind, pts, oflg, ocn_nreg, mer_nreg, nflg, regflg, minlat, maxlat) &
         bind(C, name='blomgpu_dia_set_mertra')
      import :: c_ptr, c_int
      type(c_ptr), value :: c, mtlat, nind, pts, oflg, nflg, regflg, minlat, maxlat
      integer(c_int), value :: lmax, ocn_nreg, mer_nreg
    end function
    integer(c_int) function blomgpu_dia_set_sections(c, sec_num, nsi, pts, equat_sec) bind(C, name='blomgpu_dia_set_sections')
      import :: c_ptr, c_int
      type(c_ptr), value :: c, nsi, pts
      integer(c_int), value :: sec_num, equat_sec
    end function
    integer(c_int) function blomgpu_dia_reduce(c) bind(C, name='blomgpu_dia_reduce')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_dia_msc_get(c, name, out, cap, dims) bind(C, name='blomgpu_dia_msc_get')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c, out
      character(kind=c_char), intent(in) :: name(*)
      integer(c_int), value :: cap
      integer(c_int), intent(out) :: dims(3)
    end function
    integer(c_int) function blomgpu_field_info(c, name, nlev, isint) bind(C, name='blomgpu_field_info')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      integer(c_int), intent(out) :: nlev, isint
    end function
    integer(c_int) function blomgpu_stage(c, stage, m, n, mm, nn, k1m, k1n) bind(C, name='blomgpu_stage')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: stage(*)
      integer(c_int), value :: m, n, mm, nn, k1m, k1n
    end function
    integer(c_int) function blomgpu_xctilr(c, name, lev0, l1, ld, mh, nh, itype) bind(C, name='blomgpu_xctilr')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      integer(c_int), value :: lev0, l1, ld, mh, nh, itype
    end function
    integer(c_int) function blomgpu_crc(c, name, lev0, nlev, itype, crc) bind(C, name='blomgpu_crc')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      integer(c_int), value :: lev0, nlev, itype
      integer(c_int), intent(out) :: crc
    end function
    integer(c_int) function blomgpu_xcsum(c, name, lev, itype, s) bind(C, name='blomgpu_xcsum')
      import :: c_ptr, c_int, c_char, c_double
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      integer(c_int), value :: lev, itype
      real(c_double), intent(out) :: s
    end function
    integer(c_int) function blomgpu_budget_sums(c, ncall, n, nn) bind(C, name='blomgpu_budget_sums')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
      integer(c_int), value :: ncall, n, nn
    end function
    integer(c_int) function blomgpu_budget_get(c, which, ncall, n, v) bind(C, name='blomgpu_budget_get')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: c
      integer(c_int), value :: which, ncall, n
      real(c_double), intent(out) :: v
    end function
    integer(c_int) function blomgpu_budget_init(c) bind(C, name='blomgpu_budget_init')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_budget_output(c, m) bind(C, name='blomgpu_budget_output')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
      integer(c_int), value :: m
    end function
    integer(c_int) function blomgpu_budget_steps(c, first, count) bind(C, name='blomgpu_budget_steps')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
      integer(c_int), intent(out) :: first, count
    end function
    integer(c_int) function blomgpu_budget_files(c, mask) bind(C, name='blomgpu_budget_files')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
      integer(c_int), intent(out) :: mask
    end function
    integer(c_int) function blomgpu_budget_line(c, nstep, file, terms, nterms) bind(C, name='blomgpu_budget_line')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: c
      integer(c_int), value :: nstep, file
      real(c_double), intent(out) :: terms(*)
      integer(c_int), intent(out) :: nterms
    end function
    integer(c_int) function blomgpu_sync(c) bind(C, name='blomgpu_sync')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_set_vector(c, name, v, nv) bind(C, name='blomgpu_set_vector')
      import :: c_ptr, c_int, c_char, c_double
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      real(c_double), intent(in) :: v(*)
      integer(c_int), value :: nv
    end function
    integer(c_int) function blomgpu_rccl_unique_id(id128) bind(C, name='blomgpu_rccl_unique_id')
      import :: c_int, c_char
      character(kind=c_char) :: id128(128)
    end function
    integer(c_int) function blomgpu_rccl_init_2d(c, id128, rank, npx, npy) bind(C, name='blomgpu_rccl_init_2d')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: id128(128)
      integer(c_int), value :: rank, npx, npy
    end function
    integer(c_int) function blomgpu_rccl_attach_barotp_global(c, g, isizes, jsizes) bind(C, name='blomgpu_rccl_attach_barotp_global')
      import :: c_ptr, c_int
      type(c_ptr), value :: c, g
      integer(c_int), intent(in) :: isizes(*), jsizes(*)
    end function
    ! the general tile table of xcspmd (phy/mod_xc.F90:1332-1720): i0_pe / ii_pe hold npx*npy entries, m fastest
    integer(c_int) function blomgpu_rccl_init_table(c, id128, rank, npx, npy, i0_pe, ii_pe, j0_pe, jj_pe) &
        bind(C, name='blomgpu_rccl_init_table')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: id128(128)
      integer(c_int), value :: rank, npx, npy
      integer(c_int), intent(in) :: i0_pe(*), ii_pe(*), j0_pe(*), jj_pe(*)
    end function
    integer(c_int) function blomgpu_rccl_attach_barotp_table(c, g, npx, npy, i0_pe, ii_pe, j0_pe, jj_pe) &
        bind(C, name='blomgpu_rccl_attach_barotp_table')
      import :: c_ptr, c_int
      type(c_ptr), value :: c, g
      integer(c_int), value :: npx, npy
      integer(c_int), intent(in) :: i0_pe(*), ii_pe(*), j0_pe(*), jj_pe(*)
    end function
    integer(c_int) function blomgpu_group_create_table(npx, npy, itdm, jtdm, i0_pe, ii_pe, j0_pe, jj_pe, grp) &
        bind(C, name='blomgpu_group_create_table')
      import :: c_ptr, c_int
      integer(c_int), value :: npx, npy, itdm, jtdm
      integer(c_int), intent(in) :: i0_pe(*), ii_pe(*), j0_pe(*), jj_pe(*)
      type(c_ptr), intent(out) :: grp
    end function
    integer(c_int) function blomgpu_rccl_finalize(c) bind(C, name='blomgpu_rccl_finalize')
      import :: c_ptr, c_int
      type(c_ptr), value :: c
    end function
    integer(c_int) function blomgpu_rccl_crc(c, name, lev0, nlev, itype, crc) bind(C, name='blomgpu_rccl_crc')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: c
      character(kind=c_char), intent(in) :: name(*)
      integer(c_int), value :: lev0, nlev, itype
      integer(c_int), intent(out) :: crc
    end function
  end interface

  public :: gpu_init_tile, gpu_upload_global, gpu_upload_int_global, gpu_nlev_global, gpu_rccl_unique_id, gpu_rccl_init, &
            gpu_attach_barotp_global, gpu_rccl_init_table, gpu_attach_barotp_table
  public :: gpu_init, gpu_finalize, gpu_set, gpu_upload, gpu_upload_int, gpu_download, gpu_nlev, &
            gpu_halo, gpu_chksum, gpu_sync, gpu_xcsum, budget_init, budget_sums, budget_output, gpu_budget
  public :: stage6
  public :: init_fluxes, tmsmt1, tmsmt2, advect, pbcor1, pbcor2, diffus, pgforc, momtum, &
            diapfl, barotp, eddtra, convec, sfcstr, updtrc, init_cppm, halo_cmnfld2, halo_difest, mxlayr_tail, &
            cmnfld1, cmnfld2, ale_regrid_remap, ale_vdifft, ale_vdiffm, ale_forcing, &
            cmnfld_bfsqi_ale, gpu_set_vector, difest_isobml, thermf, mxlayr, diaacc, ale_remap_diazlv
  public :: gpu_dia_select, gpu_dia_get, gpu_dia_finalize, gpu_dia_reset, gpu_dia_nacc, gpu_dia_name_ext, gpu_dia_alarm
  public :: inifrc_cesm, getfrc_cesm, gpu_cesm_nflxdi, gpu_upload_level
  public :: inifrc_ben02, gpu_ben02_ntda, gpu_ben02_reset_tda
  public :: iniswa, updswa, fwbbal, chkvar
  public :: gpu_dia_set_levels, gpu_dia_default_levels, gpu_dia_levitus2x, gpu_dia_get_levels
  public :: gpu_dia_set_sigdia, gpu_dia_clear_sigdia, gpu_dia_get_sigdia
  public :: gpu_dia_set_mertra, gpu_dia_set_sections, gpu_dia_reduce, gpu_dia_msc

  interface gpu_set
    module procedure gpu_set_real, gpu_set_int, gpu_set_str
  end interface

contains

  function cz(s) result(z)
    character(len=*), intent(in) :: s
    character(kind=c_char, len=len_trim(s)+1) :: z
    z = trim(s)//c_null_char
  end function

  subroutine gpu_check(rc, where)
    integer(c_int), intent(in) :: rc
    character(len=*), intent(in) :: where
    call gpu_check_on(ctx, rc, where)
  end subroutine

  subroutine gpu_check_on(c, rc, where)
    ! the reference prints to lp and calls xchalt + stop '(name)' (phy/mod_xc.F90:516)
    type(c_ptr), intent(in) :: c
    integer(c_int), intent(in) :: rc
    character(len=*), intent(in) :: where
    character(kind=c_char), pointer :: msg(:)
    type(c_ptr) :: p
    integer :: i
    if (rc == 0) return
    p = blomgpu_last_error(c)
    call c_f_pointer(p, msg, [512])
    i = 1
    do while (i < 512 .and. msg(i) /= c_null_char)
      i = i+1
    end do
    write (*,*) '**************************************************'
    write (*,*) msg(1:i-1)
    write (*,*) '**************************************************'
    error stop '('//where//')'
  end subroutine

  subroutine gpu_init(idm_, jdm_, kdm_, ntr_, nreg_, device)
    integer, intent(in) :: idm_, jdm_, kdm_, ntr_, nreg_, device
    type(blomgpu_dims) :: d
    idm = idm_; jdm = jdm_; kdm = kdm_; ntr = ntr_; nreg = nreg_
    itdm = idm; jtdm = jdm; i0 = 0; j0 = 0
    d = blomgpu_dims(idm, jdm, kdm, nbdy, idm, jdm, 0, 0, nreg, ntr, device)
    call gpu_check(blomgpu_create(d, ctx), 'gpu_init')
  end subroutine

  ! One tile of the itdm_ x jtdm_ grid (xcspmd, phy/mod_xc.F90:1332-2027): this process owns the points i0_+1..i0_+ii,
  ! j0_+1..j0_+jj.  idm, jdm become the tile's extents, so that gpu_upload / gpu_download keep the reference's tile-local
  ! shape a(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,:).  Also creates the second context of the whole domain that the replicated
  ! barotropic solve runs on: itdm_ x jtdm_, kdm = 3 (2-D fields only), no tracers (blom_amd/tiles.py: make_barotp_global).
  subroutine gpu_init_tile(itdm_, jtdm_, kdm_, ntr_, nreg_, i0_, j0_, ii, jj, device)
    integer, intent(in) :: itdm_, jtdm_, kdm_, ntr_, nreg_, i0_, j0_, ii, jj, device
    type(blomgpu_dims) :: d
    integer(c_int) :: rc
    idm = ii; jdm = jj; kdm = kdm_; ntr = ntr_; nreg = nreg_
    itdm = itdm_; jtdm = jtdm_; i0 = i0_; j0 = j0_
    d = blomgpu_dims(idm, jdm, kdm, nbdy, itdm, jtdm, i0, j0, nreg, ntr, device)
    call gpu_check(blomgpu_create(d, ctx), 'gpu_init_tile')
    d = blomgpu_dims(itdm, jtdm, 3, nbdy, itdm, jtdm, 0, 0, nreg, 0, device)
    rc = blomgpu_create(d, gctx)
    call gpu_check_on(gctx, rc, 'gpu_init_tile (global context)')
  end subroutine

  ! 128-byte RCCL unique id (rank 0 creates it, the launcher hands it to the others)
  subroutine gpu_rccl_unique_id(id)
    character(kind=c_char), intent(out) :: id(128)
    if (blomgpu_rccl_unique_id(id) /= 0) error stop '(gpu_rccl_unique_id: ncclGetUniqueId failed)'
  end subroutine

  ! join the communicator as tile (px, py) = (mod(rank,npx), rank/npx) of the npx x npy grid
  subroutine gpu_rccl_init(id, rank, npx, npy)
    character(kind=c_char), intent(in) :: id(128)
    integer, intent(in) :: rank, npx, npy
    call gpu_check(blomgpu_rccl_init_2d(ctx, id, rank, npx, npy), 'gpu_rccl_init')
    on_rccl = .true.
  end subroutine

  ! from now on barotp (and thermf's global sums) run on the global context; isizes / jsizes: the tile columns' widths and
  ! the tile rows' heights
  subroutine gpu_attach_barotp_global(isizes, jsizes)
    integer, intent(in) :: isizes(:), jsizes(:)
    call gpu_check(blomgpu_rccl_attach_barotp_global(ctx, gctx, isizes, jsizes), 'gpu_attach_barotp_global')
  end subroutine

  ! the same two with the general tile table of xcspmd (ragged rows, eliminated tiles): i0_pe(m,n), ii_pe(m,n) as the
  ! reference holds them (phy/mod_xc.F90:1332-1720), j0_pe(n), jj_pe(n); rank counts the non-empty tiles, m fastest
  subroutine gpu_rccl_init_table(id, rank, i0_pe, ii_pe, j0_pe, jj_pe)
    character(kind=c_char), intent(in) :: id(128)
    integer, intent(in) :: rank, i0_pe(:,:), ii_pe(:,:), j0_pe(:), jj_pe(:)
    call gpu_check(blomgpu_rccl_init_table(ctx, id, rank, size(ii_pe, 1), size(ii_pe, 2), i0_pe, ii_pe, j0_pe, jj_pe), &
                   'gpu_rccl_init_table')
    on_rccl = .true.
  end subroutine

  subroutine gpu_attach_barotp_table(i0_pe, ii_pe, j0_pe, jj_pe)
    integer, intent(in) :: i0_pe(:,:), ii_pe(:,:), j0_pe(:), jj_pe(:)
    call gpu_check(blomgpu_rccl_attach_barotp_table(ctx, gctx, size(ii_pe, 1), size(ii_pe, 2), i0_pe, ii_pe, j0_pe, jj_pe), &
                   'gpu_attach_barotp_table')
  end subroutine

  subroutine gpu_finalize()
    integer(c_int) :: rc
    if (on_rccl) rc = blomgpu_rccl_finalize(ctx)
    on_rccl = .false.
    if (c_associated(gctx)) rc = blomgpu_destroy(gctx)    ! first: it runs on the tile's stream
    gctx = c_null_ptr
    rc = blomgpu_destroy(ctx)
    ctx = c_null_ptr
  end subroutine

  subroutine gpu_set_real(name, v)
    character(len=*), intent(in) :: name
    real(8), intent(in) :: v
    call gpu_check(blomgpu_set_real(ctx, cz(name), v), 'gpu_set')
  end subroutine
  subroutine gpu_set_int(name, v)
    character(len=*), intent(in) :: name
    integer, intent(in) :: v
    call gpu_check(blomgpu_set_int(ctx, cz(name), v), 'gpu_set')
    if (name == 'difest_live') difest_estimates = v /= 0
  end subroutine
  subroutine gpu_set_str(name, v)
    character(len=*), intent(in) :: name, v
    call gpu_check(blomgpu_set_str(ctx, cz(name), cz(v)), 'gpu_set')
  end subroutine

  integer function gpu_nlev(name, isint)
    character(len=*), intent(in) :: name
    logical, intent(out) :: isint
    integer(c_int) :: nl, ii_
    call gpu_check(blomgpu_field_info(ctx, cz(name), nl, ii_), 'gpu_nlev')
    gpu_nlev = nl
    isint = ii_ /= 0
  end function

  ! the global context: levels of a field, 0 when it does not register `name`
  integer function gpu_nlev_global(name, isint)
    character(len=*), intent(in) :: name
    logical, intent(out) :: isint
    integer(c_int) :: nl, ii_
    gpu_nlev_global = 0
    isint = .false.
    if (blomgpu_field_info(gctx, cz(name), nl, ii_) /= 0) return
    gpu_nlev_global = nl
    isint = ii_ /= 0
  end function
  subroutine gpu_upload_global(name, a, nlev)
    character(len=*), intent(in) :: name
    integer, intent(in) :: nlev
    real(8), intent(in) :: a(1-nbdy:itdm+nbdy,1-nbdy:jtdm+nbdy,nlev)
    call gpu_check_on(gctx, blomgpu_upload(gctx, cz(name), a, nlev), 'gpu_upload_global')
  end subroutine
  subroutine gpu_upload_int_global(name, a, nlev)
    character(len=*), intent(in) :: name
    integer, intent(in) :: nlev
    integer, intent(in) :: a(1-nbdy:itdm+nbdy,1-nbdy:jtdm+nbdy,nlev)
    call gpu_check_on(gctx, blomgpu_upload(gctx, cz(name), a, nlev), 'gpu_upload_int_global')
  end subroutine

  ! a(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,nlev): the reference's module-array layout
  subroutine gpu_upload(name, a, nlev)
    character(len=*), intent(in) :: name
    integer, intent(in) :: nlev
    real(8), intent(in) :: a(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,nlev)
    call gpu_check(blomgpu_upload(ctx, cz(name), a, nlev), 'gpu_upload')
  end subroutine
  subroutine gpu_upload_int(name, a, nlev)
    character(len=*), intent(in) :: name
    integer, intent(in) :: nlev
    integer, intent(in) :: a(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,nlev)
    call gpu_check(blomgpu_upload(ctx, cz(name), a, nlev), 'gpu_upload_int')
  end subroutine
  subroutine gpu_download(name, a, nlev)
    character(len=*), intent(in) :: name
    integer, intent(in) :: nlev
    real(8), intent(out) :: a(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,nlev)
    call gpu_check(blomgpu_download(ctx, cz(name), a, nlev), 'gpu_download')
  end subroutine

  ! xctilr(a(1-nbdy,1-nbdy,lev0), l1, ld, mh, nh, itype), phy/mod_xc.F90:2342
  subroutine gpu_halo(name, lev0, l1, ld, mh, nh, itype)
    character(len=*), intent(in) :: name
    integer, intent(in) :: lev0, l1, ld, mh, nh, itype
    call gpu_check(blomgpu_xctilr(ctx, cz(name), lev0, l1, ld, mh, nh, itype), 'xctilr')
  end subroutine

  ! chksum(a, kcsd, itype, text), phy/mod_checksum.F90:41-74; on RCCL tiles a collective (every rank calls it) that gives
  ! the whole domain's xccrc (phy/mod_xc.F90:2195-2322), printed by the first rank only
  subroutine gpu_chksum(name, kcsd, itype, text)
    character(len=*), intent(in) :: name, text
    integer, intent(in) :: kcsd, itype
    integer(c_int) :: crc
    if (on_rccl) then
      call gpu_check(blomgpu_rccl_crc(ctx, cz(name), 1, kcsd, itype, crc), 'chksum')
    else
      call gpu_check(blomgpu_crc(ctx, cz(name), 1, kcsd, itype, crc), 'chksum')
    end if
    if (mnproc == 1) write (*,'(3a,z8.8)') ' chksum: ', trim(text), ': 0x', crc
  end subroutine

  subroutine gpu_xcsum(s, name, lev, itype)    ! phy/mod_xc.F90:4116 xcsum(sum, a, mask) on a device field
    real(c_double), intent(out) :: s
    character(len=*), intent(in) :: name
    integer, intent(in) :: lev, itype
    call gpu_check(blomgpu_xcsum(ctx, cz(name), lev, itype, s), 'xcsum')
  end subroutine
  subroutine budget_sums(ncall, n, nn)         ! phy/mod_budget.F90:95
    integer, intent(in) :: ncall, n, nn
    call gpu_check(blomgpu_budget_sums(ctx, ncall, n, nn), 'budget_sums')
  end subroutine
  subroutine budget_init()                     ! phy/mod_budget.F90:73 (nothing unless gpu_set('cnsvdi', 1))
    call gpu_check(blomgpu_budget_init(ctx), 'budget_init')
  end subroutine
  ! phy/mod_budget.F90:198: the sums sf tf trf of this step into its record, and -- on rank 1, once the step before has a record, the
  ! reference's nstep > nstep1 + 1 -- the step's line appended to each of salbud tembud tkebud glsbud trcbud trcbudtot that the tracer
  ! set calls for (:213-268), the numbers blomgpu_budget_line evaluates in the reference's order
  subroutine budget_output(m)
    integer, intent(in) :: m
    character(len=9), parameter :: files(0:5) = [character(len=9) :: 'salbud', 'tembud', 'tkebud', 'glsbud', 'trcbud', 'trcbudtot']
    integer(c_int) :: first, count, nterms, mask
    real(c_double) :: terms(7)
    integer :: f, nfu, nstep
    call gpu_check(blomgpu_budget_output(ctx, m), 'budget_output')
    call gpu_check(blomgpu_budget_steps(ctx, first, count), 'budget_output')
    if (mnproc /= 1 .or. count < 2) return     ! (count = 0: cnsvdi is off)
    nstep = first+count-1
    call gpu_check(blomgpu_budget_files(ctx, mask), 'budget_output')
    do f = 0, 5
      if (.not. btest(mask, f)) cycle                      ! a file the tracer set does not call for (:231-268)
      call gpu_check(blomgpu_budget_line(ctx, nstep, f, terms, nterms), 'budget_output')
      open (newunit = nfu, file = trim(files(f)), position = 'append')
      if (nterms == 7) then
        write (nfu, '(i8,7e18.10)') nstep-1, terms(1:7)
      else
        write (nfu, '(i8,6e12.4)') nstep-1, terms(1:6)
      end if
      close (nfu)
    end do
  end subroutine
  function gpu_budget(which, ncall, n) result(v)   ! sdp/tdp/trdp/tkedp/glsdp(ncall,n), phy/mod_budget.F90:49-57
    integer, intent(in) :: which, ncall, n
    real(c_double) :: v
    call gpu_check(blomgpu_budget_get(ctx, which, ncall, n, v), 'budget_get')
  end function

  subroutine gpu_sync()
    call gpu_check(blomgpu_sync(ctx), 'gpu_sync')
  end subroutine

  subroutine stage6(name, m, n, mm, nn, k1m, k1n)
    character(len=*), intent(in) :: name
    integer, intent(in) :: m, n, mm, nn, k1m, k1n
    call gpu_check(blomgpu_stage(ctx, cz(name), m, n, mm, nn, k1m, k1n), name)
  end subroutine

  ! ---- stage API of the reference ------------------------------------------------------------
  subroutine init_fluxes(m,n,mm,nn,k1m,k1n)   ! phy/mod_state.F90:341
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('init_fluxes',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine tmsmt1(nn)                        ! phy/mod_tmsmt.F90:209
    integer, intent(in) :: nn
    call stage6('tmsmt1',0,0,0,nn,0,0)
  end subroutine
  subroutine tmsmt2(m,mm,nn,k1m)               ! phy/mod_tmsmt.F90:281
    integer, intent(in) :: m,mm,nn,k1m
    call stage6('tmsmt2',m,0,mm,nn,k1m,0)
  end subroutine
  subroutine advect(m,n,mm,nn,k1m,k1n)         ! phy/mod_advect.F90:59
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('advect',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine pbcor1(m,n,mm,nn,k1m,k1n)         ! phy/mod_pbcor.F90:66
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('pbcor1',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine pbcor2(m,n,mm,nn,k1m,k1n)         ! phy/mod_pbcor.F90:416
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('pbcor2',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine diffus(m,n,mm,nn,k1m,k1n)         ! phy/mod_diffus.F90:41
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('diffus',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine pgforc(m,n,mm,nn,k1m,k1n)         ! phy/mod_pgforc.F90:438
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('pgforc',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine momtum(m,n,mm,nn,k1m,k1n)         ! phy/mod_momtum.F90:215
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('momtum',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine diapfl(n,nn,k1n)                  ! phy/mod_diapfl.F90:49
    integer, intent(in) :: n,nn,k1n
    call stage6('diapfl',0,n,0,nn,0,k1n)
  end subroutine
  subroutine barotp(m,n,mm,nn,k1m,k1n)         ! phy/mod_barotp.F90:148
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('barotp',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine updtrc(m,n,mm,nn,k1m,k1n)         ! trc/mod_tracers_update.F90:152
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('updtrc',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine sfcstr(m,n,mm,nn,k1m,k1n)         ! phy/mod_sfcstr.F90:33
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('sfcstr',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine convec(m,n,mm,nn,k1m,k1n)         ! phy/mod_convec.F90:43
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('convec',m,n,mm,nn,k1m,k1n)
  end subroutine

  subroutine eddtra(m,n,mm,nn,k1m,k1n)         ! phy/mod_eddtra.F90:148
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('eddtra',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine init_cppm()                       ! phy/mod_cppm.F90:2504
    call stage6('init_cppm',0,0,0,0,0,0)
  end subroutine
  subroutine halo_cmnfld2(n)                   ! phy/mod_cmnfld_routines.F90:1171-1196
    integer, intent(in) :: n
    call stage6('halo_cmnfld2',0,n,0,0,0,0)
  end subroutine
  subroutine cmnfld1(m,n,mm,nn,k1m,k1n)         ! phy/mod_cmnfld_routines.F90:1090 (isopyc_bulkml: cmnfld_z)
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('cmnfld1',m,n,mm,nn,k1m,k1n)
  end subroutine cmnfld1
  ! diaacc (phy/mod_dia.F90:1092, called at phy/mod_blom_step.F90:239): the accumulators selected with gpu_dia_select; without a
  ! selection it does nothing
  subroutine diaacc(m,n,mm,nn,k1m,k1n)
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('diaacc',m,n,mm,nn,k1m,k1n)
  end subroutine diaacc
  ! the selection: a blank-separated list of the reference's ACC_* suffixes in lower case ('temp saln uvel sealv'), '' for none;
  ! replaces the previous one, adds diaini's dependencies (phy/mod_dia.F90:598-608), initialises as inifld does
  subroutine gpu_dia_select(names)
    character(len=*), intent(in) :: names
    call gpu_check(blomgpu_dia_select(ctx, cz(names)), 'gpu_dia_select')
  end subroutine
  ! the accumulator on the tile's padded plane(s): nlev = 1 for a 2-D name, kdm for a layer name, ddm for a depth-level name
  ! (phyh2d / phylyr / phylvl of the reference)
  subroutine gpu_dia_get(name, a, nlev)
    character(len=*), intent(in) :: name
    integer, intent(in) :: nlev
    real(8), intent(out) :: a(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,nlev)
    call gpu_check(blomgpu_dia_get(ctx, cz(name), a), 'gpu_dia_get')
  end subroutine
  ! row `index` (0-based) of the whole accumulator table, the column-derived rows included (blomgpu_dia_name_ext): the name, its
  ! kind (0 2-D, 1 kdm layers, 2 ddm depth levels, 3 kdm density classes, 4 internal) and grid (0 p, 1 u, 2 v); found = .false.
  ! behind the last row
  subroutine gpu_dia_name_ext(index, name, kind, grid, found)
    integer, intent(in) :: index
    character(len=*), intent(out) :: name
    integer, intent(out) :: kind, grid
    logical, intent(out) :: found
    character(kind=c_char) :: buf(32)
    integer(c_int) :: k, g
    integer :: q
    name = ' '
    kind = -1
    grid = -1
    found = blomgpu_dia_name_ext(int(index, c_int), buf, 32_c_int, k, g) == 0
    if (.not. found) return
    kind = k
    grid = g
    do q = 1, min(32, len(name))
      if (buf(q) == c_null_char) exit
      name(q:q) = buf(q)
    end do
  end subroutine gpu_dia_name_ext
  subroutine gpu_dia_finalize()                 ! finlyr for the weighted layer pairs, phy/mod_dia.F90:2597-2611
    call gpu_check(blomgpu_dia_finalize(ctx), 'gpu_dia_finalize')
  end subroutine
  subroutine gpu_dia_reset()                    ! inifld, phy/mod_dia.F90:5864
    call gpu_check(blomgpu_dia_reset(ctx), 'gpu_dia_reset')
  end subroutine
  ! alarm_phy(1) of the one output group, 0 or 1: under cntiso_hybrid / plevel templvl salnlvl uvellvl vvellvl take their sample inside
  ! ale_regrid_remap while it is 0 (phy/mod_ale_regrid_remap.F90:1524-1531), in ale_remap_diazlv when it is 1 (:2014-2017)
  subroutine gpu_dia_alarm(alarm)
    integer, intent(in) :: alarm
    call gpu_check(blomgpu_dia_alarm(ctx, int(alarm, c_int)), 'gpu_dia_alarm')
  end subroutine
  ! The coupled experiment (expcnf = 'cesm').  inifrc_cesm (cesm/mod_cesm.F90:175-200) is also the declaration that the coupler's forcing
  ! exists: until it has been called sfcstr and thermf refuse expcnf = 'cesm'.  getfrc_cesm: cesm/mod_cesm.F90:202-263.
  subroutine inifrc_cesm()
    call gpu_check(blomgpu_inifrc_cesm(ctx), 'inifrc_cesm')
  end subroutine
  subroutine gpu_upload_level(name, a, lev)      ! one level of a field: a(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) into level lev
    character(len=*), intent(in) :: name
    integer, intent(in) :: lev
    real(8), intent(in) :: a(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy)
    call gpu_check(blomgpu_upload_level(ctx, cz(name), a, int(lev, c_int)), 'gpu_upload_level')
  end subroutine
  subroutine getfrc_cesm()
    call gpu_check(blomgpu_getfrc_cesm(ctx), 'getfrc_cesm')
  end subroutine
  subroutine gpu_cesm_nflxdi(nflxdi)            ! mod_forcing's nflxdi
    integer, intent(out) :: nflxdi(48)
    integer(c_int) :: n(48)
    call gpu_check(blomgpu_cesm_nflxdi(ctx, n), 'gpu_cesm_nflxdi')
    nflxdi = int(n)
  end subroutine
  ! The end of blom_step (phy/mod_blom_step.F90:96-252), each with the reference's call line; updswa, fwbbal and chkvar return at once
  ! unless their options (swamth, sprfac, chkvar) have declared them.
  ! iniswa (phy/mod_swabs.F90:216): for the method gpu_set('swamth', ...) names.  chl: the monthly chlorophyll concentration the
  ! reference reads from ccfile, for the chlorophyll methods -- log10 where it is positive inside the tile (:391-402), uploaded as
  ! chl10c, halos updated (:405).
  subroutine iniswa(chl)
    real(8), intent(in), optional :: chl(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,12)
    real(8), allocatable :: c10(:,:,:)
    integer :: i, j, k
    call gpu_check(blomgpu_iniswa(ctx), 'iniswa')
    if (.not. present(chl)) return
    allocate(c10(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,12))
    c10 = chl
    do k = 1, 12
      do j = 1, jdm
        do i = 1, idm
          if (c10(i,j,k) > 0._8) c10(i,j,k) = log10(c10(i,j,k))
        end do
      end do
    end do
    call gpu_upload('chl10c', c10, 12)
    call gpu_halo('chl10c', 1, 1, 12, nbdy, nbdy, 1)
    deallocate(c10)
  end subroutine
  ! updswa (phy/mod_swabs.F90:611); with csdiag the four checksum lines of :722-730, which the chlorophyll methods alone reach
  subroutine updswa(csdiag)
    logical, intent(in), optional :: csdiag
    integer(c_int) :: nl, ii_
    call gpu_check(blomgpu_updswa(ctx), 'updswa')
    if (.not. present(csdiag)) return
    if (.not. csdiag) return
    if (blomgpu_field_info(ctx, cz('chl10'), nl, ii_) /= 0) return
    if (mnproc == 1) write (*,*) 'updswa:'
    call gpu_chksum('swfc1', 1, 1, 'swfc1')
    call gpu_chksum('swfc2', 1, 1, 'swfc2')
    call gpu_chksum('swal1', 1, 1, 'swal1')
    call gpu_chksum('swal2', 1, 1, 'swal2')
  end subroutine
  subroutine fwbbal(m,n,mm,nn,k1m,k1n)              ! phy/mod_forcing.F90:361
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call gpu_check(blomgpu_fwbbal(ctx, m, n, mm, nn, k1m, k1n), 'fwbbal')
  end subroutine
  subroutine chkvar(m,n,mm,nn,k1m,k1n)              ! phy/mod_chkvar.F90:77
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call gpu_check(blomgpu_chkvar(ctx, m, n, mm, nn, k1m, k1n), 'chkvar')
  end subroutine
  ! The forced ocean-ice experiment (expcnf = 'ben02clim' / 'ben02syn' / 'single_column').  inifrc_ben02 declares that its forcing
  ! exists: until it has been called sfcstr and thermf refuse these experiments.  asflux stays the host's: it reads the five _tda planes
  ! and gpu_ben02_ntda, uploads its fluxes by name, and calls gpu_ben02_reset_tda (ben02/mod_ben02.F90:1623-1624, :1701-1705).
  subroutine inifrc_ben02()
    call gpu_check(blomgpu_inifrc_ben02(ctx), 'inifrc_ben02')
  end subroutine
  subroutine gpu_ben02_ntda(ntda)               ! mod_ben02's ntda
    integer, intent(out) :: ntda
    integer(c_int) :: n
    call gpu_check(blomgpu_ben02_ntda(ctx, n), 'gpu_ben02_ntda')
    ntda = int(n)
  end subroutine
  subroutine gpu_ben02_reset_tda()
    call gpu_check(blomgpu_ben02_reset_tda(ctx), 'gpu_ben02_reset_tda')
  end subroutine
  ! the depth levels of the *lvl names as depthslev_bnds(2,ddm) (phy/mod_dia.F90:119-128); refused while a *lvl name is selected
  subroutine gpu_dia_set_levels(bnds, ddm)
    integer, intent(in) :: ddm
    real(8), intent(in), target :: bnds(2,ddm)
    call gpu_check(blomgpu_dia_set_levels(ctx, c_loc(bnds), int(ddm, c_int)), 'gpu_dia_set_levels')
  end subroutine
  subroutine gpu_dia_default_levels()           ! the 35 levels of phy/mod_dia.F90:111-128
    call gpu_check(blomgpu_dia_set_levels(ctx, c_null_ptr, 0_c_int), 'gpu_dia_default_levels')
  end subroutine
  subroutine gpu_dia_levitus2x()                ! the 70 levels of LEVITUS2X, :130-159
    call gpu_check(blomgpu_dia_levels_levitus2x(ctx), 'gpu_dia_levitus2x')
  end subroutine
  subroutine gpu_dia_get_levels(bnds, cap, ddm) ! ddm, and the first min(cap, ddm) levels' bounds
    integer, intent(in) :: cap
    real(8), intent(out), target :: bnds(2,cap)
    integer, intent(out) :: ddm
    integer(c_int) :: v
    call gpu_check(blomgpu_dia_get_levels(ctx, c_loc(bnds), int(cap, c_int), v), 'gpu_dia_get_levels')
    ddm = v
  end subroutine
  ! the diagnostic density classes sigdia(kdm) (phy/mod_vcoord.F90:978-1005) of the class names umfll umfltdl umflsml vmfll vmfltdl
  ! vmflsml (phy/mod_dia.F90:1368-1538); before the selection, refused while a class name is selected
  subroutine gpu_dia_set_sigdia(sigdia, n)
    integer, intent(in) :: n
    real(8), intent(in), target :: sigdia(n)
    call gpu_check(blomgpu_dia_set_sigdia(ctx, c_loc(sigdia), int(n, c_int)), 'gpu_dia_set_sigdia')
  end subroutine
  subroutine gpu_dia_clear_sigdia()
    call gpu_check(blomgpu_dia_set_sigdia(ctx, c_null_ptr, 0_c_int), 'gpu_dia_clear_sigdia')
  end subroutine
  subroutine gpu_dia_get_sigdia(sigdia, cap, n) ! n (0: no table), and the first min(cap, n) values
    integer, intent(in) :: cap
    real(8), intent(out), target :: sigdia(cap)
    integer, intent(out) :: n
    integer(c_int) :: v
    call gpu_check(blomgpu_dia_get_sigdia(ctx, c_loc(sigdia), int(cap, c_int), v), 'gpu_dia_get_sigdia')
    n = v
  end subroutine
  integer function gpu_dia_nacc()               ! nacc_phy
    integer(c_int) :: v
    call gpu_check(blomgpu_dia_nacc(ctx, v), 'gpu_dia_nacc')
    gpu_dia_nacc = v
  end function
  ! diaout_iogrp's reductions (phy/mod_dia.F90:2366-2588).  The tables diamer reads from mer_orfile and mer_mifile (:4026-4108) and
  ! diasec from sec_sifile (:3838-3866) are the host's: pts(4,n) = (i, j, uflg, vflg) per point, oflg(itdm,jtdm), regflg(20,mer_nreg)
  ! (Fortran order: the C arrays' transposes).  gpu_dia_reduce goes where diaout_iogrp has diamer and diasec: behind the last step of
  ! the window (and ale_remap_diazlv), in front of gpu_dia_finalize; gpu_dia_msc hands one result out with its extents (:4113-4119).
  subroutine gpu_dia_set_mertra(lmax, mtlat, nind, pts, oflg, ocn_nreg, mer_nreg, nflg, regflg, minlat, maxlat)
    integer, intent(in) :: lmax, ocn_nreg, mer_nreg
    real(8), intent(in), target :: mtlat(lmax), minlat(mer_nreg), maxlat(mer_nreg)
    integer(c_int), intent(in), target :: nind(lmax), pts(4,*), oflg(*), nflg(mer_nreg), regflg(20,mer_nreg)
    call gpu_check(blomgpu_dia_set_mertra(ctx, int(lmax, c_int), c_loc(mtlat), c_loc(nind), c_loc(pts), c_loc(oflg), int(ocn_nreg, c_int), &
         int(mer_nreg, c_int), c_loc(nflg), c_loc(regflg), c_loc(minlat), c_loc(maxlat)), 'gpu_dia_set_mertra')
  end subroutine
  subroutine gpu_dia_set_sections(sec_num, nsi, pts, equat_sec)
    integer, intent(in) :: sec_num, equat_sec
    integer(c_int), intent(in), target :: nsi(sec_num), pts(4,*)
    call gpu_check(blomgpu_dia_set_sections(ctx, int(sec_num, c_int), c_loc(nsi), c_loc(pts), int(equat_sec, c_int)), 'gpu_dia_set_sections')
  end subroutine
  subroutine gpu_dia_reduce()
    call gpu_check(blomgpu_dia_reduce(ctx), 'gpu_dia_reduce')
  end subroutine
  subroutine gpu_dia_msc(name, a, cap, dims)
    character(len=*), intent(in) :: name
    integer, intent(in) :: cap
    real(8), intent(out), target :: a(cap)
    integer, intent(out) :: dims(3)
    integer(c_int) :: d(3)
    call gpu_check(blomgpu_dia_msc_get(ctx, cz(name), c_loc(a), int(cap, c_int), d), 'gpu_dia_msc')
    dims = d
  end subroutine
  subroutine cmnfld2(m,n,mm,nn,k1m,k1n)         ! phy/mod_cmnfld_routines.F90:1158 (halo updates, bfsqf, neutral slopes)
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('cmnfld2',m,n,mm,nn,k1m,k1n)
  end subroutine cmnfld2
  subroutine halo_difest(nn)                   ! phy/mod_difest.F90:750-772
    integer, intent(in) :: nn
    call stage6('halo_difest',0,0,0,nn,0,0)
  end subroutine
  subroutine difest_isobml(m,n,mm,nn,k1m,k1n)   ! phy/mod_difest.F90:735
    ! difest_estimates = .true.: the whole routine (difest_common_iso, difest_vertical_iso, difest_lateral_iso: difint, difiso, difdia,
    ! difwgt estimated every step) -- the host must have uploaded what they read beside the state: plat, cosang, sinang, twedon, ficem,
    ! buoyfl, the planes tdmls and bdmlq its own libm fills (include/blomgpu.h) and &DIFFUSION's variables through gpu_set;
    ! .false. (default): the part in front of the estimates, :750-790
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    if (difest_estimates) then
      call stage6('difest_isobml',m,n,mm,nn,k1m,k1n)
    else
      call stage6('difest_isobml_pre',m,n,mm,nn,k1m,k1n)
    end if
  end subroutine
  subroutine thermf(m,n,mm,nn,k1m,k1n)          ! phy/mod_thermf.F90:35
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('thermf',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine mxlayr(m,n,mm,nn,k1m,k1n)          ! phy/mod_mxlayr.F90:130
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('mxlayr',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine mxlayr_tail(nn,k1n)               ! phy/mod_mxlayr.F90:1266-1310
    integer, intent(in) :: nn,k1n
    call stage6('mxlayr_tail',0,0,0,nn,0,k1n)
  end subroutine
  subroutine ale_regrid_remap(m,n,mm,nn,k1m,k1n)   ! phy/mod_ale_regrid_remap.F90:1486 (vcoord 'plevel', 'cntiso_hybrid'/'direct')
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('ale_regrid_remap',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine ale_remap_diazlv(m,n,mm,nn,k1m,k1n)   ! phy/mod_ale_regrid_remap.F90:1986; called where blom_step does, phy/mod_blom_step.F90:271-273
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('ale_remap_diazlv',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine ale_vdifft(m,n,mm,nn,k1m,k1n)          ! phy/mod_ale_vdiff.F90:50
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('ale_vdifft',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine ale_vdiffm(m,n,mm,nn,k1m,k1n)          ! phy/mod_ale_vdiff.F90:245
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('ale_vdiffm',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine cmnfld_bfsqi_ale(m,n,mm,nn,k1m,k1n)    ! phy/mod_cmnfld_routines.F90:352
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('cmnfld_bfsqi_ale',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine ale_forcing(m,n,mm,nn,k1m,k1n)         ! phy/mod_ale_forcing.F90:45
    integer, intent(in) :: m,n,mm,nn,k1m,k1n
    call stage6('ale_forcing',m,n,mm,nn,k1m,k1n)
  end subroutine
  subroutine gpu_set_vector(name, v)           ! 1-D module arrays: 'plevel' (phy/mod_vcoord.F90:99)
    character(len=*), intent(in) :: name
    real(c_double), intent(in) :: v(:)
    call gpu_check(blomgpu_set_vector(ctx, cz(name), v, size(v)), name)
  end subroutine

end module mod_blomgpu

! ------------------------------------------------------------------------------
! mod_xcspmd_gpu -- the tile table of the reference, patch.input, as xcspmd reads
! and checks it (phy/mod_xc.F90:1332-1540; format in the comment block :1405-1430):
!
!   npes   npe   mpe   idm   jdm  ibig  jbig  nreg ...
!      8     4     2   180   193    45    97     2 ...
!   ispt(  1) =      1    46    91   136          (first i-point of every tile of tile row 1)
!   iipe(  1) =     45    45    45    45          (their i-extents)
!   ...                                           (one ispt/iipe pair per tile row, mpe rows)
!   jspt(  1) =      1    98                      (first j-point of every tile row)
!   jjpe(  1) =     97    96                      (their j-extents)
!
! Only tensor-product layouts are carried (every tile row cut alike, no empty
! tiles): land-tile elimination is not supported (blom_amd/tiles.py says the same).
! A layout that does not fit is refused with the reason, before any RCCL call, and
! every rank refuses it alike -- no rank is left waiting for a peer.
! ------------------------------------------------------------------------------
module mod_xcspmd_gpu

  implicit none
  private
  public :: xcspmd_gpu

contains

  subroutine refuse(msg)
    character(len=*), intent(in) :: msg
    write (*,'(a)') ' xcspmd: '//trim(msg)
    error stop '(xcspmd)'
  end subroutine

  ! reads `fname` and checks it against the rank count and the state's dimensions; isizes(npe) / jsizes(mpe): the widths
  ! of the tile columns and the heights of the tile rows
  subroutine xcspmd_gpu(fname, world, idm, jdm, nreg, nbdy, isizes, jsizes)
    character(len=*), intent(in) :: fname
    integer, intent(in) :: world, idm, jdm, nreg, nbdy
    integer, allocatable, intent(out) :: isizes(:), jsizes(:)
    integer, allocatable :: ispt(:,:), iipe(:,:), jspt(:), jjpe(:)
    logical, allocatable :: seen(:,:)
    character(len=1024) :: line
    character(len=160) :: msg
    character(len=4) :: key
    integer :: u, ios, npes, npe, mpe, pidm, pjdm, ibig, jbig, pnreg, n, m, k, p, q
    open (newunit=u, file=fname, status='old', action='read', iostat=ios)
    if (ios /= 0) call refuse('cannot open '//trim(fname))
    read (u, '(a)', iostat=ios) line                    ! the column names
    read (u, *, iostat=ios) npes, npe, mpe, pidm, pjdm, ibig, jbig, pnreg
    if (ios /= 0) call refuse(trim(fname)//': the second line must hold npes npe mpe idm jdm ibig jbig nreg')
    write (msg, '(a,i0,a,i0)') 'patch.input is for npes = ', npes, ' ranks but WORLD_SIZE = ', world
    if (npes /= world) call refuse(msg)
    write (msg, '(a,i0,a,i0,a,i0)') 'npe x mpe = ', npe, ' x ', mpe, ' is not npes = ', npes
    if (npe < 1 .or. mpe < 1 .or. npe*mpe /= npes) call refuse(msg)
    allocate (ispt(npe,mpe), iipe(npe,mpe), jspt(mpe), jjpe(mpe), seen(2,mpe+1))
    seen = .false.
    do
      read (u, '(a)', iostat=ios) line
      if (ios /= 0) exit
      line = adjustl(line)
      if (len_trim(line) == 0) cycle
      key = line(1:4)
      p = index(line, '(')
      q = index(line, ')')
      k = index(line, '=')
      if (p /= 5 .or. q < p .or. k < q) call refuse(trim(fname)//': cannot read the line "'//trim(line)//'"')
      read (line(p+1:q-1), *, iostat=ios) n
      if (ios /= 0) call refuse(trim(fname)//': cannot read the line "'//trim(line)//'"')
      select case (key)
        case ('ispt', 'iipe')
          if (n < 1 .or. n > mpe) call refuse(trim(fname)//': tile row out of range in "'//trim(line)//'"')
          if (key == 'ispt') then
            read (line(k+1:), *, iostat=ios) ispt(:,n)
          else
            read (line(k+1:), *, iostat=ios) iipe(:,n)
          end if
          seen(merge(1, 2, key == 'ispt'), n) = ios == 0
        case ('jspt', 'jjpe')
          if (n /= 1) call refuse(trim(fname)//': only jspt(1) / jjpe(1) are read')
          if (key == 'jspt') then
            read (line(k+1:), *, iostat=ios) jspt
          else
            read (line(k+1:), *, iostat=ios) jjpe
          end if
          seen(merge(1, 2, key == 'jspt'), mpe+1) = ios == 0
        case default
          call refuse(trim(fname)//': unexpected line "'//trim(line)//'"')
      end select
      if (ios /= 0) call refuse(trim(fname)//': too few values in "'//trim(line)//'"')
    end do
    close (u)
    if (.not. all(seen)) call refuse(trim(fname)//': an ispt/iipe line of a tile row or jspt/jjpe is missing')

    if (any(iipe <= 0) .or. any(jjpe <= 0)) &
      call refuse('empty tile (iipe or jjpe = 0): land-tile elimination is not supported')
    do n = 2, mpe
      if (any(iipe(:,n) /= iipe(:,1)) .or. any(ispt(:,n) /= ispt(:,1))) &
        call refuse('the tile rows are cut differently (land-tile elimination / a non-tensor-product layout is not supported)')
    end do
    do m = 1, npe
      if (ispt(m,1) /= 1+sum(iipe(1:m-1,1))) call refuse('decomposition is non-contiguous (ispt)')
    end do
    do n = 1, mpe
      if (jspt(n) /= 1+sum(jjpe(1:n-1))) call refuse('decomposition is non-contiguous (jspt)')
    end do
    write (msg, '(a,i0,a,i0,a,i0,a,i0)') 'the tiles cover ', sum(iipe(:,1)), ' x ', sum(jjpe), &
                                        ' points but the state is idm x jdm = ', idm, ' x ', jdm
    if (sum(iipe(:,1)) /= idm .or. sum(jjpe) /= jdm) call refuse(msg)
    write (msg, '(a,i0,a,i0,a,i0,a,i0)') 'patch.input has idm x jdm = ', pidm, ' x ', pjdm, ' but the state is ', idm, ' x ', jdm
    if (pidm /= idm .or. pjdm /= jdm) call refuse(msg)
    write (msg, '(a,i0,a,i0)') 'patch.input has nreg = ', pnreg, ' but the state has nreg = ', nreg
    if (pnreg /= nreg) call refuse(msg)
    ! arctic patch: every tile of the top row as wide as itdm/ipr (:1483-1505)
    if (nreg == 2 .and. npe > 1) then
      write (msg, '(a,i0)') 'arctic tiles are not the right size: they should have ii = itdm/npe = ', idm/npe
      if (any(iipe(:,mpe) /= idm/npe) .or. mod(idm, npe) /= 0) call refuse(msg)
    end if
    write (msg, '(a,i0,a)') 'a tile is narrower than nbdy = ', nbdy, ' points'
    if (any(iipe < nbdy) .or. any(jjpe < nbdy)) call refuse(msg)
    isizes = iipe(:,1)
    jsizes = jjpe
  end subroutine

end module mod_xcspmd_gpu
