! ------------------------------------------------------------------------------
! program blom_dyncore -- standalone Fortran driver of the device-resident
! dynamical core, in the shape of the reference's `program blom`
! (drivers/nocoupler/blom.F:20-66): initialise, loop blom_step until the last step,
! print the final field checksum of dp (blom.F:56-57), write 'success' to run.status.
!
! Options: the reference's `limits` namelist file (mod_rdlim_gpu.F90).
! Initial state: a raw binary dump (blom_amd/statefile.py writes it from the numpy host
! initialisation); the reference reads netCDF here, which is out of scope.
!   record 1: idm jdm kdm ntr nreg nsteps  (int32 x6), baclin (real64)
!   then per entry: name (16 chars), kind (int32: 0 real field, 1 int field, 2 real option,
!                   3 int option, 4 string option), nlev (int32), payload
!
! As N ranks (INTEGRATION.md, "Running as N ranks"): every rank runs this program, as every rank of
! the reference runs `program blom`.  The rank environment is torchrun's (RANK, WORLD_SIZE, LOCAL_RANK;
! the device is LOCAL_RANK); a tile table `patch.input` in the working directory (read as xcspmd reads
! it, mod_xcspmd_gpu) switches tiles on, a 1x1 table on one rank included.  Every rank reads the whole
! state file and keeps its window; the RCCL id travels from rank 0 through the file $BLOM_RCCL_ID_FILE.
! ------------------------------------------------------------------------------
program blom_dyncore

  use iso_c_binding, only: c_char, c_int, c_null_char
  use mod_blomgpu
  use mod_xcspmd_gpu, only: xcspmd_gpu
  use mod_rdlim_gpu, only: rdlim_gpu, hybrid_coordinate, advect_cppm
  implicit none

  interface
    integer(c_int) function c_rename(old, new) bind(C, name='rename')
      import :: c_int, c_char
      character(kind=c_char), intent(in) :: old(*), new(*)
    end function
    integer(c_int) function c_usleep(us) bind(C, name='usleep')
      import :: c_int
      integer(c_int), value :: us
    end function
    integer(c_int) function c_getppid() bind(C, name='getppid')
      import :: c_int
    end function
  end interface

  character(len=256) :: fname
  character(len=16)  :: name
  character(len=32)  :: sval
  character(len=512) :: idfile
  character(kind=c_char) :: rccl_id(128)
  integer :: u, ios, kind, nlev, nsteps, nstep, nstep1, nstep2, i4(6), ival
  integer :: rank, world, local_rank, npx, npy, px, py
  real(8) :: baclin, rval
  logical :: have_limits, full_physics = .false., tiled, isint
  integer, allocatable :: isizes(:), jsizes(:)
  real(8), allocatable :: buf(:,:,:)
  integer, allocatable :: ibuf(:,:,:)

  rank = env_int('RANK', 0)
  world = env_int('WORLD_SIZE', 1)
  local_rank = env_int('LOCAL_RANK', 0)
  if (world < 1 .or. rank < 0 .or. rank >= world) error stop '(blom_dyncore: RANK must lie in 0 .. WORLD_SIZE-1)'
  call get_command_argument(1, fname)
  if (len_trim(fname) == 0) fname = 'blom_state.bin'
  open (newunit=u, file=trim(fname), access='stream', form='unformatted', status='old', action='read')
  read (u) i4, baclin
  nsteps = i4(6)
  ! xcspmd: the tile table decides the layout; everything is checked before any RCCL call, alike on every rank
  inquire (file='patch.input', exist=tiled)
  if (tiled) then
    call xcspmd_gpu('patch.input', world, i4(1), i4(2), i4(5), nbdy, isizes, jsizes)
    npx = size(isizes)
    npy = size(jsizes)
    px = mod(rank, npx)                            ! rank = px + npx*py (blomgpu_rccl_init_2d)
    py = rank/npx
    call gpu_init_tile(i4(1), i4(2), i4(3), i4(4), i4(5), sum(isizes(1:px)), sum(jsizes(1:py)), isizes(px+1), jsizes(py+1), &
                       local_rank)
    mnproc = rank+1
    npes = world
  else
    if (world /= 1) then
      write (*,'(a,i0,a)') ' blom_dyncore: WORLD_SIZE = ', world, ' but no patch.input in the working directory'
      error stop '(xcspmd)'
    end if
    call gpu_init(i4(1), i4(2), i4(3), i4(4), i4(5), local_rank)
  end if
  ! each rank reads the whole state: a tile takes the window i0+1..i0+idm+2*nbdy, j0+1..j0+jdm+2*nbdy of every padded field
  ! (its halo included, so that no halo update is needed before the first step; blom_amd/tiles.py: TileLayout.window); the
  ! global context of the barotropic solve takes the whole masks and every real field of <= 3 levels it registers alike
  do
    read (u, iostat=ios) name, kind, nlev
    if (ios /= 0) exit
    select case (kind)
      case (0)
        allocate (buf(itdm+2*nbdy, jtdm+2*nbdy, nlev))
        read (u) buf
        call gpu_upload(trim(name), buf(i0+1:i0+idm+2*nbdy, j0+1:j0+jdm+2*nbdy, :), nlev)
        if (tiled .and. nlev <= 3) then
          if (gpu_nlev_global(trim(name), isint) == nlev .and. .not. isint) call gpu_upload_global(trim(name), buf, nlev)
        end if
        deallocate (buf)
      case (1)
        allocate (ibuf(itdm+2*nbdy, jtdm+2*nbdy, nlev))
        read (u) ibuf
        call gpu_upload_int(trim(name), ibuf(i0+1:i0+idm+2*nbdy, j0+1:j0+jdm+2*nbdy, :), nlev)
        if (tiled .and. (name == 'ip' .or. name == 'iu' .or. name == 'iv' .or. name == 'iq')) &
          call gpu_upload_int_global(trim(name), ibuf, nlev)
        deallocate (ibuf)
      case (2)
        read (u) rval
        call gpu_set(trim(name), rval)
      case (3)
        read (u) ival
        call gpu_set(trim(name), ival)
        ! config 2's step as far as the device library has it (thermf, mxlayr, the front of difest_isobml, cmnfld2, cmnfld1):
        ! the host sequences the stages itself, so it needs to know
        if (trim(name) == 'full_physics') full_physics = ival /= 0
      case (4)
        read (u) sval
        call gpu_set(trim(name), trim(sval))
    end select
  end do
  close (u)
  ! options: the reference's namelist file `limits` / `ocn_in` in the working directory, when there is one, decides them
  ! (rdlim, phy/mod_rdlim.F90:137-175) and the length of the run; the option records of the state file are the fall-back
  nstep1 = 0
  nstep2 = nsteps
  call rdlim_gpu(have_limits, nstep1, nstep2, baclin)
  call get_command_argument(2, sval)               ! optional: stop after this many steps (short test runs)
  if (len_trim(sval) > 0) then
    read (sval, *) nsteps
    nstep2 = nstep1+nsteps
  end if
  ! thermf's ocean area (mod_grid: area) is the option record of the state file: the whole domain's, the same on every rank
  if (tiled) then
    call share_rccl_id(rccl_id)
    call gpu_rccl_init(rccl_id, rank, npx, npy)
    call gpu_attach_barotp_global(isizes, jsizes)
  end if

  ! the step counter starts at nstep1 = nday1*nstep_in_day (its parity decides the time levels and the order of cppm's sweeps)
  nstep = nstep1
  if (advect_cppm) call init_cppm()
  call budget_init()                               ! phy/mod_blom_init.F90 (nothing unless cnsvdi)
  if (hybrid_coordinate) then
    ! blom_init's cmnfld1 (phy/mod_blom_init.F90): the mixed layer depth the first eddtra and ale_forcing read
    ! with blom_init's time level indices (phy/mod_blom_init.F90:256-261: m = mod(nstep1+1,2)+1, n = mod(nstep1,2)+1)
    call cmnfld1(mod(nstep+1,2)+1, mod(nstep,2)+1, mod(nstep+1,2)*kdm, mod(nstep,2)*kdm, 1+mod(nstep+1,2)*kdm, 1+mod(nstep,2)*kdm)
  end if
  do while (nstep < nstep2)
    call blom_step(nstep)
  end do

  call gpu_sync()
  ! collectives on tiles: every rank calls them, the first prints (blom.F:56-57)
  call gpu_chksum('dp', 2*kdm, 1, 'dp')
  call gpu_chksum('temp', 2*kdm, 1, 'temp')
  call gpu_chksum('u', 2*kdm, 13, 'u')
  if (difest_estimates) call gpu_chksum('difint', kdm, 1, 'difint')     ! (the estimates ran: see mod_blomgpu)
  if (mnproc == 1) then
    open (newunit=u, file='run.status', status='unknown')
    write (u,*) 'success'                          ! blom.F:59-61
    close (u)
  end if
  call gpu_finalize()
  if (tiled .and. world > 1 .and. rank == 0) then  ! every rank has read the id: the checksums needed all of them
    open (newunit=u, file=trim(idfile), status='old', iostat=ios)
    if (ios == 0) close (u, status='delete')
  end if

contains

  integer function env_int(var, default)
    character(len=*), intent(in) :: var
    integer, intent(in) :: default
    character(len=32) :: v
    integer :: st
    env_int = default
    call get_environment_variable(var, v, status=st)
    if (st /= 0 .or. len_trim(v) == 0) return
    read (v, *, iostat=st) env_int
    if (st /= 0) then
      write (*,'(4a)') ' blom_dyncore: ', var, ' is not an integer: ', trim(v)
      error stop '(blom_dyncore)'
    end if
  end function

  ! The RCCL unique id, rank 0 -> every rank, without MPI: rank 0 writes the 128 bytes and a run token to $BLOM_RCCL_ID_FILE
  ! (default ./blom_rccl_id) under a temporary name and renames it; the others wait for it (300 s at most) and take it only
  ! when its token is theirs, so that a file an earlier run left behind is never joined.  The token is $BLOM_RUN_TOKEN, or
  ! else the parent process and torchrun's restart count -- the ranks of one launch are children of one launcher.
  subroutine share_rccl_id(id)
    character(kind=c_char), intent(out) :: id(128)
    character(len=128) :: token, got
    character(len=32) :: v
    integer :: f, st, waited
    logical :: ex
    call get_environment_variable('BLOM_RCCL_ID_FILE', idfile, status=st)
    if (st /= 0 .or. len_trim(idfile) == 0) idfile = 'blom_rccl_id'
    call get_environment_variable('BLOM_RUN_TOKEN', token, status=st)
    if (st /= 0 .or. len_trim(token) == 0) then
      call get_environment_variable('TORCHELASTIC_RESTART_COUNT', v, status=st)
      if (st /= 0) v = '0'
      write (token, '(a,i0,2a)') 'ppid ', c_getppid(), ' restart ', trim(v)
    end if
    if (world == 1) then
      call gpu_rccl_unique_id(id)
      return
    end if
    if (rank == 0) then
      call gpu_rccl_unique_id(id)
      open (newunit=f, file=trim(idfile)//'.tmp', access='stream', form='unformatted', status='replace', action='write', iostat=st)
      if (st == 0) write (f, iostat=st) id, token
      if (st == 0) close (f, iostat=st)
      if (st /= 0) then
        write (*,'(2a)') ' blom_dyncore: cannot write ', trim(idfile)//'.tmp'
        error stop '(blom_dyncore)'
      end if
      if (c_rename(trim(idfile)//'.tmp'//c_null_char, trim(idfile)//c_null_char) /= 0) then
        write (*,'(2a)') ' blom_dyncore: cannot rename the id file to ', trim(idfile)
        error stop '(blom_dyncore)'
      end if
      return
    end if
    waited = 0
    do
      inquire (file=trim(idfile), exist=ex)
      if (ex) then
        open (newunit=f, file=trim(idfile), access='stream', form='unformatted', status='old', action='read', iostat=st)
        if (st == 0) then
          read (f, iostat=st) id, got
          close (f)
          if (st == 0 .and. got == token) return
        end if
      end if
      if (waited >= 300000) then
        if (ex) then
          write (*,'(3a)') ' blom_dyncore: ', trim(idfile), ' is from another run (its token differs) and rank 0 wrote none in 300 s'
        else
          write (*,'(3a)') ' blom_dyncore: no RCCL id from rank 0 in ', trim(idfile), ' after 300 s'
        end if
        error stop '(blom_dyncore)'
      end if
      st = c_usleep(50000_c_int)
      waited = waited+50
    end do
  end subroutine

  subroutine blom_step(nstep)
    ! stage sequence of phy/mod_blom_step.F90:89-253, dynamical core only
    integer, intent(inout) :: nstep
    integer :: m, n, mm, nn, k1m, k1n
    m = mod(nstep  ,2)+1
    n = mod(nstep+1,2)+1
    mm = (m-1)*kdm
    nn = (n-1)*kdm
    k1m = 1+mm
    k1n = 1+nn
    nstep = nstep+1                                ! step_time
    call gpu_set('nstep', nstep)
    if (hybrid_coordinate) then
      ! vcoord_type = 'cntiso_hybrid' or 'plevel', phy/mod_blom_step.F90:126-233 as far as the device library has it
      ! (DESIGN.md 3h; difest_*_hybrid and thermf are left out: what they produce stays as uploaded)
      call budget_sums(1,n,nn)                     ! phy/mod_blom_step.F90:96 (nothing unless cnsvdi)
      call init_fluxes(m,n,mm,nn,k1m,k1n)
      call updswa()                                ! phy/mod_blom_step.F90:122 (nothing without a chlorophyll swamth)
      call tmsmt1(nn)
      call ale_regrid_remap(m,n,mm,nn,k1m,k1n)
      call budget_sums(2,n,nn)
      call cmnfld2(m,n,mm,nn,k1m,k1n)
      call stage6('halo_difest_hyb',m,n,mm,nn,k1m,k1n)
      call eddtra(m,n,mm,nn,k1m,k1n)
      call advect(m,n,mm,nn,k1m,k1n)
      call pbcor1(m,n,mm,nn,k1m,k1n)
      call diffus(m,n,mm,nn,k1m,k1n)
      call budget_sums(3,n,nn)
      call sfcstr(m,n,mm,nn,k1m,k1n)
      call pgforc(m,n,mm,nn,k1m,k1n)
      call momtum(m,n,mm,nn,k1m,k1n)
      call cmnfld_bfsqi_ale(m,n,mm,nn,k1m,k1n)
      call ale_forcing(m,n,mm,nn,k1m,k1n)
      call stage6('halo_difest_vert',m,n,mm,nn,k1m,k1n)
      call ale_vdifft(m,n,mm,nn,k1m,k1n)
      call ale_vdiffm(m,n,mm,nn,k1m,k1n)
      call budget_sums(4,n,nn)
      call updtrc(m,n,mm,nn,k1m,k1n)
      call budget_sums(5,n,nn)
      call barotp(m,n,mm,nn,k1m,k1n)
      call pbcor2(m,n,mm,nn,k1m,k1n)
      call budget_sums(6,m,mm)
      call tmsmt2(m,mm,nn,k1m)
      call budget_sums(7,m,mm)
      call cmnfld1(m,n,mm,nn,k1m,k1n)
      call diaacc(m,n,mm,nn,k1m,k1n)               ! phy/mod_blom_step.F90:239 (nothing without gpu_dia_select)
      call fwbbal(m,n,mm,nn,k1m,k1n)               ! :242 (nothing without sprfac)
      call budget_output(m)                        ! :245
      call chkvar(m,n,mm,nn,k1m,k1n)               ! :252 (nothing without the option chkvar)
      call gpu_set('delt1', baclin+baclin)
      return
    end if
    if (full_physics) then
      ! phy/mod_blom_step.F90:96-253 for isopyc_bulkml, every stage the device library has (DESIGN.md 3i); of difest_isobml the
      ! part in front of the diffusivity estimates
      call budget_sums(1,n,nn)                     ! phy/mod_blom_step.F90:96 (nothing unless cnsvdi)
      call init_fluxes(m,n,mm,nn,k1m,k1n)
      call updswa()                                ! phy/mod_blom_step.F90:122 (nothing without a chlorophyll swamth)
      call tmsmt1(nn)
      call cmnfld2(m,n,mm,nn,k1m,k1n)
      call difest_isobml(m,n,mm,nn,k1m,k1n)
      call eddtra(m,n,mm,nn,k1m,k1n)
      call advect(m,n,mm,nn,k1m,k1n)
      call pbcor1(m,n,mm,nn,k1m,k1n)
      call diffus(m,n,mm,nn,k1m,k1n)
      call budget_sums(2,n,nn)
      call sfcstr(m,n,mm,nn,k1m,k1n)
      call pgforc(m,n,mm,nn,k1m,k1n)
      call momtum(m,n,mm,nn,k1m,k1n)
      call convec(m,n,mm,nn,k1m,k1n)
      call budget_sums(3,n,nn)
      call diapfl(n,nn,k1n)
      call budget_sums(4,n,nn)
      call thermf(m,n,mm,nn,k1m,k1n)
      call mxlayr(m,n,mm,nn,k1m,k1n)
      call updtrc(m,n,mm,nn,k1m,k1n)
      call budget_sums(5,n,nn)
      call barotp(m,n,mm,nn,k1m,k1n)
      call pbcor2(m,n,mm,nn,k1m,k1n)
      call budget_sums(6,m,mm)
      call tmsmt2(m,mm,nn,k1m)
      call budget_sums(7,m,mm)
      call cmnfld1(m,n,mm,nn,k1m,k1n)
      call diaacc(m,n,mm,nn,k1m,k1n)               ! phy/mod_blom_step.F90:239 (nothing without gpu_dia_select)
      call fwbbal(m,n,mm,nn,k1m,k1n)               ! :242 (nothing without sprfac)
      call budget_output(m)                        ! :245
      call chkvar(m,n,mm,nn,k1m,k1n)               ! :252 (nothing without the option chkvar)
      call gpu_set('delt1', baclin+baclin)
      return
    end if
    call budget_sums(1,n,nn)                     ! phy/mod_blom_step.F90:96 (nothing unless cnsvdi)
    call init_fluxes(m,n,mm,nn,k1m,k1n)
    call updswa()                                  ! phy/mod_blom_step.F90:122 (nothing without a chlorophyll swamth)
    call tmsmt1(nn)
    call halo_cmnfld2(n)
    call halo_difest(nn)
    call eddtra(m,n,mm,nn,k1m,k1n)
    call advect(m,n,mm,nn,k1m,k1n)
    call pbcor1(m,n,mm,nn,k1m,k1n)
    call diffus(m,n,mm,nn,k1m,k1n)
    call budget_sums(2,n,nn)
    call sfcstr(m,n,mm,nn,k1m,k1n)
    call pgforc(m,n,mm,nn,k1m,k1n)
    call momtum(m,n,mm,nn,k1m,k1n)
    call convec(m,n,mm,nn,k1m,k1n)
    call budget_sums(3,n,nn)
    call diapfl(n,nn,k1n)
    call budget_sums(4,n,nn)
    call mxlayr_tail(nn,k1n)
    call updtrc(m,n,mm,nn,k1m,k1n)
    call budget_sums(5,n,nn)
    call barotp(m,n,mm,nn,k1m,k1n)
    call pbcor2(m,n,mm,nn,k1m,k1n)
    call budget_sums(6,m,mm)
    call tmsmt2(m,mm,nn,k1m)
    call budget_sums(7,m,mm)
    call diaacc(m,n,mm,nn,k1m,k1n)                 ! phy/mod_blom_step.F90:239 (nothing without gpu_dia_select)
    call fwbbal(m,n,mm,nn,k1m,k1n)                 ! :242 (nothing without sprfac)
    call budget_output(m)                        ! :245
    call chkvar(m,n,mm,nn,k1m,k1n)                 ! :252 (nothing without the option chkvar)
    call gpu_set('delt1', baclin+baclin)           ! phy/mod_blom_step.F90:300
  end subroutine blom_step

end program blom_dyncore
