! Driver for tests/golden/make_stepend_golden.py: runs the reference's own iniswa / updswa (phy/mod_swabs.F90), fwbbal
! (phy/mod_forcing.F90) or chkvar (phy/mod_chkvar.F90) behind the stand-ins of stepend_standins.F90 on inputs read from in.bin, and writes
! what they leave to out.bin.  This project's own text.  control.txt: the mode, then that mode's scalars.
program stepend_driver
  use mod_xc
  use mod_time
  implicit none
  integer :: mode
  open (11, file='control.txt', status='old')
  open (12, file='in.bin', access='stream', form='unformatted', status='old')
  open (13, file='out.bin', access='stream', form='unformatted', status='replace')
  read (11,*) mode
  read (12) ip
  call segments()
  select case (mode)
    case (1)
      call run_swabs()
    case (2)
      call run_fwbbal()
    case (3)
      call run_chkvar()
  end select
  close (13)
contains
  subroutine run_swabs()
    use mod_swabs, only: swamth, chlopt, jwtype, swfc1, swfc2, swal1, swal2, iniswa, updswa
    use netcdf, only: chl
    real :: fill
    integer :: nset, q
    read (11,'(a)') swamth
    read (11,*) jwtype, fill, nset
    chlopt = 'climatology'
    read (12) chl
    swfc1 = fill; swfc2 = fill + 1.; swal1 = fill + 2.; swal2 = fill + 3.
    call iniswa()
    write (13) swfc1, swfc2, swal1, swal2
    do q = 1, nset
      read (11,*) l1mi, l2mi, l3mi, l4mi, l5mi, xmi
      call updswa()
      write (13) swfc1, swfc2, swal1, swal2
    end do
  end subroutine run_swabs
  subroutine run_fwbbal()
    use mod_forcing, only: sprfac, prfac, eiacc, pracc, eva, fmltfz, lip, sop, rnf, rfi, fwbbal
    use mod_grid, only: scp2
    integer :: nsteps, q
    read (11,*) nstep_in_day, baclin, nsteps
    read (12) ipwocn
    read (12) scp2, eva, fmltfz, lip, sop, rnf, rfi, eiacc, pracc
    sprfac = .true.
    prfac = 1.
    do q = 1, nsteps
      read (11,*) nday_of_year, nstep
      call fwbbal(1, 2, 0, kk, 1, 1 + kk)
      write (13) eiacc, pracc, prfac
    end do
  end subroutine run_fwbbal
  subroutine run_chkvar()
    use mod_state, only: dp, temp, saln
    use mod_chkvar, only: chkvar
    integer :: n
    read (11,*) n
    read (12) dp, temp, saln
    call chkvar(3 - n, n, (2 - n)*kk, (n - 1)*kk, 1 + (2 - n)*kk, 1 + (n - 1)*kk)
    write (*,'(a)') ' chkvar: clean'
  end subroutine run_chkvar
end program stepend_driver
