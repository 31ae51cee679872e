! Stand-in modules for compiling the reference's cesm/mod_thermf_cesm.F90 on its own (tests/golden/make_thermf_cesm_golden.py).
! This project's own text: each module declares only the names thermf_cesm uses, with the reference's shapes.  Dimensions come from
! the preprocessor (-DIDM= -DJDM= -DKDM= -DNTR=).  xcsum follows phy/mod_xc.F90:4116-4161: strips of 2*nbdy+1 points along a row, the
! strip sums added to the row sum in order, the row sums added serially.
module mod_xc
  implicit none
  integer, parameter :: nbdy = 4, idm = IDM, jdm = JDM, kdm = KDM, ms = 16
  integer, parameter :: ii = idm, jj = jdm, kk = kdm, mnproc = 1, lp = 6, halo_ps = 1
  integer, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: ip, ips, ipwocn
  integer, dimension(1-nbdy:jdm+nbdy) :: isp
  integer, dimension(1-nbdy:jdm+nbdy,ms) :: ifp, ilp
contains
  subroutine xcsum(total, a, mask)
    real, intent(out) :: total
    real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy), intent(in) :: a
    integer, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy), intent(in) :: mask
    real :: row(jdm), strip
    integer :: i, i1, j
    do j = 1, jdm
      row(j) = 0.
      do i1 = 1, idm, 2*nbdy+1
        strip = 0.
        do i = i1, min(i1+2*nbdy, idm)
          if (mask(i,j) == 1) strip = strip + a(i,j)
        end do
        row(j) = row(j) + strip
      end do
    end do
    total = row(1)
    do j = 2, jdm
      total = total + row(j)
    end do
  end subroutine xcsum
  subroutine segments()
    ! the wet segments of each row, from ip (what bigrid leaves in isp, ifp, ilp)
    integer :: i, j
    do j = 1-nbdy, jdm+nbdy
      isp(j) = 0
      do i = 1-nbdy, idm+nbdy
        if (ip(i,j) == 1) then
          if (i == 1-nbdy) then
            isp(j) = isp(j) + 1
            ifp(j,isp(j)) = i
          else if (ip(i-1,j) /= 1) then
            isp(j) = isp(j) + 1
            ifp(j,isp(j)) = i
          end if
          ilp(j,isp(j)) = i
        end if
      end do
    end do
  end subroutine segments
end module mod_xc

module mod_time
  implicit none
  integer :: nstep, nstep_in_day, nday_in_year, nday_of_year, l1mi, l2mi, l3mi, l4mi, l5mi
  real :: baclin, xmi
end module mod_time

module mod_vcoord
  implicit none
  integer, parameter :: vcoord_isopyc_bulkml = 1
  integer :: vcoord_tag = 1
end module mod_vcoord

module mod_grid
  use mod_xc, only: nbdy, idm, jdm
  implicit none
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: scp2
  real :: area
end module mod_grid

module mod_state
  use mod_xc, only: nbdy, idm, jdm, kdm
  implicit none
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,2*kdm) :: dp, temp, saln
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,kdm+1) :: p
end module mod_state

module mod_eos
  implicit none
  real :: atf = 0., btf = -1.8, ctf = 0.          ! what inieos sets for expcnf = 'cesm'
end module mod_eos

module mod_forcing
  use mod_xc, only: nbdy, idm, jdm, kdm
  implicit none
  real :: sref, trxday, srxday, trxdpt, srxdpt, trxlim, srxlim
  logical :: aptflx, apsflx, ditflx, disflx, srxbal, use_stream_relaxation
  integer :: nflxdi(48)
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,48) :: tflxap, sflxap, tflxdi, sflxdi
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,12) :: sstclm, ricclm, sssclm
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: swa, nsf, hmltfz, lip, sop, eva, rnf, rfi, fmltfz, sfl, ustarw, surflx, surrlx, &
    sswflx, salflx, brnflx, salrlx, ustar, salt_corr, sss_stream, sst_stream, ice_stream
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,NTR) :: trc_corr
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,kdm+1) :: t_rs_nonloc, s_rs_nonloc
end module mod_forcing

module mod_cesm
  use mod_xc, only: nbdy, idm, jdm
  implicit none
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: hmlt, frzpot, mltpot
end module mod_cesm

module mod_utility
  use mod_xc, only: nbdy, idm, jdm
  implicit none
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: util1, util2, util3
end module mod_utility

module mod_checksum
  implicit none
  logical :: csdiag = .false.
contains
  subroutine chksum(a, kcsd, halo, text)
    real, intent(in) :: a(*)
    integer, intent(in) :: kcsd, halo
    character(len=*), intent(in) :: text
  end subroutine chksum
end module mod_checksum

module mod_tracers
  use mod_xc, only: nbdy, idm, jdm, kdm
  implicit none
  integer, parameter :: ntr = NTR
  integer :: itrtke = -1, itrgls = -1
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,2*kdm,NTR) :: trc
  real, dimension(NTR,1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: trflx
end module mod_tracers

module mod_diffusion
  use mod_xc, only: nbdy, idm, jdm, kdm
  implicit none
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,kdm) :: difdia
end module mod_diffusion

module mod_tke
  implicit none
  real, parameter :: gls_cmu0 = .527, Zos = .0002, gls_p = 3., gls_m = 1.5, gls_n = -1., vonKar = .4
end module mod_tke
