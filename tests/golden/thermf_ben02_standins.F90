! Stand-in modules for compiling the reference's ben02/mod_thermf_ben02.F90 and ben02/mod_sfcstr_ben02.F90 on their own, together with its
! ben02/mod_thdysi.F90 and phy/mod_seaice.F90 (tests/golden/make_thermf_ben02_golden.py).  This project's own text: each module declares
! only the names the two routines use, with the reference's shapes.  Dimensions come from the preprocessor (-DIDM= -DJDM= -DKDM= -DNTR=).
! xcsum follows phy/mod_xc.F90:4116-4161: strips of 2*nbdy+1 points along a row, the strip sums added to the row sum in order, the row
! sums added serially.  xctilr is the single tile's halo update of a domain that is periodic in i and closed in j, which is the grid
! the generator uses.
module mod_xc
  implicit none
  integer, parameter :: nbdy = 4, idm = IDM, jdm = JDM, kdm = KDM, ms = 16
  integer, parameter :: ii = idm, jj = jdm, kk = kdm, mnproc = 1, lp = 6, halo_ps = 1, halo_uv = 13, halo_vv = 14
  real, parameter :: vland = 0.
  integer, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: ip, iu, iv, ips, ipwocn
  integer, dimension(1-nbdy:jdm+nbdy) :: isp, isu, isv
  integer, dimension(1-nbdy:jdm+nbdy,ms) :: ifp, ilp, ifu, ilu, ifv, ilv
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
  subroutine xctilr(a, l1, ld, mh, nh, itype)
    integer, intent(in) :: l1, ld, mh, nh, itype
    real, intent(inout) :: a(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,ld)
    integer :: i, j, k, q
    do k = l1, ld
      do j = 1, nh
        do i = 1, ii
          a(i,1-j,k) = vland
          a(i,jj+j,k) = vland
        end do
      end do
      do q = 1, mh
        do j = 1-nh, jj+nh
          a(1-q,j,k) = a(ii+1-q,j,k)
          a(ii+q,j,k) = a(q,j,k)
        end do
      end do
    end do
  end subroutine xctilr
  subroutine row_segments(mask, is, if, il)
    ! the wet segments of each row of a mask (what bigrid leaves in isp, ifp, ilp and their u- and v-grid kin)
    integer, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy), intent(in) :: mask
    integer, dimension(1-nbdy:jdm+nbdy), intent(out) :: is
    integer, dimension(1-nbdy:jdm+nbdy,ms), intent(out) :: if, il
    integer :: i, j
    do j = 1-nbdy, jdm+nbdy
      is(j) = 0
      do i = 1-nbdy, idm+nbdy
        if (mask(i,j) == 1) then
          if (i == 1-nbdy) then
            is(j) = is(j) + 1
            if(j,is(j)) = i
          else if (mask(i-1,j) /= 1) then
            is(j) = is(j) + 1
            if(j,is(j)) = i
          end if
          il(j,is(j)) = i
        end if
      end do
    end do
  end subroutine row_segments
  subroutine segments()
    call row_segments(ip, isp, ifp, ilp)
    call row_segments(iu, isu, ifu, ilu)
    call row_segments(iv, isv, ifv, ilv)
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
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: scp2, plat
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
  real :: atf = -0.0547, btf = 0., ctf = 0.       ! what inieos sets for expcnf = 'ben02clim', 'ben02syn', 'single_column'
end module mod_eos

module mod_forcing
  use mod_xc, only: nbdy, idm, jdm, kdm
  implicit none
  real :: sref, trxday, srxday, trxdpt, srxdpt, trxlim, srxlim
  logical :: aptflx, apsflx, ditflx, disflx, srxbal
  integer :: nflxdi(48)
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,48) :: tflxap, sflxap, tflxdi, sflxdi
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,12) :: sstclm, ricclm, sssclm
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: swa, nsf, hmltfz, lip, sop, eva, rnf, rfi, fmltfz, sfl, ustarw, surflx, surrlx, &
    sswflx, salflx, brnflx, salrlx, ustar, salt_corr, ztx, mty, taux, tauy
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,NTR) :: trc_corr
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,kdm+1) :: t_rs_nonloc, s_rs_nonloc
end module mod_forcing

module mod_swabs
  use mod_xc, only: nbdy, idm, jdm
  implicit none
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: swal2, swfc2
end module mod_swabs

module mod_ben02
  use mod_xc, only: nbdy, idm, jdm
  implicit none
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: tsi_tda, tml_tda, sml_tda, alb_tda, fice_tda, tsi, dfl, albw, alb, rnfins, rnfres
  integer :: ntda = 0, nrfets = 7
  real :: rhowat = 1024.
end module mod_ben02

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
