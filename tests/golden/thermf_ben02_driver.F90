! Driver for the reference's sfcstr_ben02 and thermf_ben02 compiled behind the stand-ins of thermf_ben02_standins.F90 (this project's own
! text).  Reads scalars from `scalars.txt` and arrays from `in.bin` (stream, native, the order below), calls sfcstr_ben02 and then
! thermf_ben02 once, writes `out.bin`.
program thermf_ben02_driver
  use mod_xc
  use mod_time
  use mod_vcoord, only: vcoord_tag
  use mod_grid, only: scp2, plat, area
  use mod_state, only: dp, temp, saln, p
  use mod_forcing
  use mod_swabs, only: swal2, swfc2
  use mod_ben02
  use mod_thdysi, only: tsrfm, ticem
  use mod_seaice, only: ficem, hicem, hsnwm, ustari, tauxice, tauyice, iagem
  use mod_utility, only: util2, util3
  use mod_tracers, only: ntr, itrtke, itrgls, trc, trflx
  use mod_diffusion, only: difdia
  use mod_sfcstr_ben02, only: sfcstr_ben02
  use mod_thermf_ben02, only: thermf_ben02
  implicit none
  integer :: m, n, mm, nn, k1m, k1n, nt, u, fl(5)
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: fill
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,NTR) :: tf
  open (newunit=u, file='scalars.txt', status='old')
  read (u,*) m, n, mm, nn, k1m, k1n
  read (u,*) nstep, nstep_in_day, nday_in_year, nday_of_year, l1mi, l2mi, l3mi, l4mi, l5mi
  read (u,*) baclin, xmi, sref, area, trxday, srxday, trxdpt, srxdpt, trxlim, srxlim
  read (u,*) fl, vcoord_tag, itrtke, itrgls, ntda
  close (u)
  aptflx = fl(1) /= 0; apsflx = fl(2) /= 0; ditflx = fl(3) /= 0; disflx = fl(4) /= 0; srxbal = fl(5) /= 0
  open (newunit=u, file='in.bin', access='stream', form='unformatted', status='old')
  read (u) ip, iu, iv, ipwocn, nflxdi
  read (u) scp2, plat, dp, temp, saln, p, trc, difdia, swfc2, swal2
  read (u) swa, nsf, dfl, lip, sop, eva, rfi, rnfins, ustarw, tsi, albw, ztx, mty, ustari, tauxice, tauyice
  read (u) ficem, hicem, hsnwm, tsrfm, iagem, rnfres, tsi_tda, tml_tda, sml_tda, alb_tda, fice_tda
  read (u) salt_corr, trc_corr, sstclm, ricclm, sssclm, tflxap, sflxap, tflxdi, sflxdi
  read (u) fill
  close (u)
  ips = ip
  call segments()
  ! the pure outputs start from the caller's pattern, so that a store to a land or halo point would be seen
  ticem = fill; alb = fill; rnf = fill; fmltfz = fill; sfl = fill; brnflx = fill; salflx = fill; hmltfz = fill; surflx = fill
  sswflx = fill; surrlx = fill; salrlx = fill; util2 = fill; util3 = fill; ustar = fill; taux = fill; tauy = fill
  do nt = 1, ntr
    trflx(nt,:,:) = fill
  end do
  do nt = 1, kk+1
    t_rs_nonloc(:,:,nt) = fill; s_rs_nonloc(:,:,nt) = fill
  end do
  call sfcstr_ben02()
  call thermf_ben02(m,n,mm,nn,k1m,k1n)
  do nt = 1, ntr
    tf(:,:,nt) = trflx(nt,:,:)
  end do
  open (newunit=u, file='out.bin', access='stream', form='unformatted', status='replace')
  write (u) ficem, hicem, hsnwm, tsrfm, ticem, alb, iagem, rnfres, tsi_tda, tml_tda, sml_tda, alb_tda, fice_tda
  write (u) rnf, fmltfz, sfl, brnflx, salflx, hmltfz, surflx, sswflx, surrlx, salrlx, util2, util3, salt_corr, ustar, taux, tauy
  write (u) tf, trc_corr, t_rs_nonloc, s_rs_nonloc, tflxdi, sflxdi
  write (u) nflxdi, ntda
  close (u)
end program thermf_ben02_driver
