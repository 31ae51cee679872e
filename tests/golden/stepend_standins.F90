! Stand-in modules for compiling the reference's phy/mod_swabs.F90, phy/mod_forcing.F90, phy/mod_chkvar.F90 and phy/mod_intp1d.F90 on
! their own (tests/golden/make_stepend_golden.py).  This project's own text: each module declares only the names the routines use, with the
! reference's shapes.  Dimensions come from the preprocessor (-DIDM= -DJDM= -DKDM= -DNTR=).  xcsum follows phy/mod_xc.F90:4116-4161:
! strips of 2*nbdy+1 points along a row, the strip sums added to the row sum in order, the row sums added serially.  xctilr is the single
! tile's halo update of a domain that is periodic in i and closed in j, which is the grid the generator uses; xcaput copies the global
! array into the tile's interior.  The netcdf module hands iniswa the driver's synthetic chlorophyll: nf90_get_var with start and count
! returns month start(3) of netcdf's chl, so that the real iniswa fills its private chl10c and tables and the real updswa runs unchanged.
! mod_time is a stand-in too: the reference's step_time needs mod_calendar's date, which init_timevars sets from a namelist file.
module dimensions
  implicit none
  integer, parameter :: idm = IDM, jdm = JDM, kdm = KDM, itdm = IDM, jtdm = JDM
end module dimensions

module mod_xc
  use dimensions
  implicit none
  integer, parameter :: nbdy = 4, ms = 16
  integer, parameter :: ii = idm, jj = jdm, kk = kdm, mnproc = 1, lp = 6, halo_ps = 1, i0 = 0, j0 = 0
  real, parameter :: vland = 0.
  integer, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: ip, ipwocn
  integer, dimension(1-nbdy:jdm+nbdy) :: isp
  integer, dimension(1-nbdy:jdm+nbdy,ms) :: ifp, ilp
contains
  subroutine xcstop(text)
    character(len=*), intent(in) :: text
  end subroutine xcstop
  subroutine xchalt(text)
    character(len=*), intent(in) :: text
  end subroutine xchalt
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
  subroutine xcaput(aa, a, mnflg)
    real, intent(in) :: aa(itdm,jtdm)
    real, intent(inout) :: a(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy)
    integer, intent(in) :: mnflg
    a(1:idm,1:jdm) = aa
  end subroutine xcaput
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
  subroutine segments()
    ! the wet segments of each row of ip (what bigrid leaves in isp, ifp, ilp)
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

module mod_grid
  use mod_xc, only: nbdy, idm, jdm
  implicit none
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: scp2
end module mod_grid

module mod_state
  use mod_xc, only: nbdy, idm, jdm, kdm
  implicit none
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,2*kdm) :: dp, temp, saln
end module mod_state

module mod_tracers
  implicit none
  integer, parameter :: ntr = NTR
end module mod_tracers

module mod_utility
  implicit none
  integer, parameter :: fnmlen = 256
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

module netcdf
  use dimensions
  implicit none
  integer, parameter :: nf90_nowrite = 0, nf90_noerr = 0
  real :: chl(itdm,jtdm,12)            ! the driver's synthetic monthly chlorophyll concentration
  interface nf90_get_var
    module procedure get_month, get_plane
  end interface
contains
  integer function nf90_open(path, mode, ncid)
    character(len=*), intent(in) :: path
    integer, intent(in) :: mode
    integer, intent(out) :: ncid
    ncid = 1
    nf90_open = nf90_noerr
  end function nf90_open
  integer function nf90_close(ncid)
    integer, intent(in) :: ncid
    nf90_close = nf90_noerr
  end function nf90_close
  function nf90_strerror(errstat)
    integer, intent(in) :: errstat
    character(len=8) :: nf90_strerror
    nf90_strerror = 'stand-in'
  end function nf90_strerror
  integer function nf90_inq_dimid(ncid, name, dimid)
    integer, intent(in) :: ncid
    character(len=*), intent(in) :: name
    integer, intent(out) :: dimid
    dimid = 3
    if (name == 'x') dimid = 1
    if (name == 'y') dimid = 2
    nf90_inq_dimid = nf90_noerr
  end function nf90_inq_dimid
  integer function nf90_inquire_dimension(ncid, dimid, len)
    integer, intent(in) :: ncid, dimid
    integer, intent(out) :: len
    len = 12
    if (dimid == 1) len = itdm
    if (dimid == 2) len = jtdm
    nf90_inquire_dimension = nf90_noerr
  end function nf90_inquire_dimension
  integer function nf90_inq_varid(ncid, name, varid)
    integer, intent(in) :: ncid
    character(len=*), intent(in) :: name
    integer, intent(out) :: varid
    varid = 1
    nf90_inq_varid = nf90_noerr
  end function nf90_inq_varid
  integer function get_month(ncid, varid, values, start, count)
    integer, intent(in) :: ncid, varid, start(3), count(3)
    real, intent(out) :: values(itdm,jtdm)
    values = chl(:,:,start(3))
    get_month = nf90_noerr
  end function get_month
  integer function get_plane(ncid, varid, values)
    integer, intent(in) :: ncid, varid
    real, intent(out) :: values(itdm,jtdm)
    values = 0.
    get_plane = nf90_noerr
  end function get_plane
end module netcdf
