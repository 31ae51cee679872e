! Driver for the reference's thermf_cesm compiled behind the stand-ins of thermf_cesm_standins.F90 (this project's own text).
! Reads scalars from `scalars.txt` and arrays from `in.bin` (stream, native, the order below), calls thermf_cesm once, writes `out.bin`.
program thermf_cesm_driver
  use mod_xc
  use mod_time
  use mod_vcoord, only: vcoord_tag
  use mod_grid, only: scp2, area
  use mod_state, only: dp, temp, saln, p
  use mod_forcing
  use mod_cesm, only: hmlt, frzpot, mltpot
  use mod_utility, only: util2, util3
  use mod_tracers, only: ntr, itrtke, itrgls, trc, trflx
  use mod_diffusion, only: difdia
  use mod_thermf_cesm, only: thermf_cesm
  implicit none
  integer :: m, n, mm, nn, k1m, k1n, nt, u, fl(6)
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy) :: fill
  real, dimension(1-nbdy:idm+nbdy,1-nbdy:jdm+nbdy,NTR) :: tf
  open (newunit=u, file='scalars.txt', status='old')
  read (u,*) m, n, mm, nn, k1m, k1n
  read (u,*) nstep, nstep_in_day, nday_in_year, nday_of_year, l1mi, l2mi, l3mi, l4mi, l5mi
  read (u,*) baclin, xmi, sref, area, trxday, srxday, trxdpt, srxdpt, trxlim, srxlim
  read (u,*) fl, vcoord_tag, itrtke, itrgls
  close (u)
  aptflx = fl(1) /= 0; apsflx = fl(2) /= 0; ditflx = fl(3) /= 0; disflx = fl(4) /= 0; srxbal = fl(5) /= 0
  use_stream_relaxation = fl(6) /= 0
  open (newunit=u, file='in.bin', access='stream', form='unformatted', status='old')
  read (u) ip, ipwocn, nflxdi
  read (u) scp2, dp, temp, saln, p, trc, difdia
  read (u) swa, nsf, hmlt, lip, sop, eva, rnf, rfi, fmltfz, sfl, ustarw, sst_stream, sss_stream, ice_stream, salt_corr, trc_corr
  read (u) sstclm, ricclm, sssclm, tflxap, sflxap, tflxdi, sflxdi
  read (u) fill
  close (u)
  ips = ip
  call segments()
  ! the outputs start from the caller's pattern, so that a store to a land or halo point would be seen
  surflx = fill; sswflx = fill; surrlx = fill; salflx = fill; brnflx = fill; salrlx = fill; hmltfz = fill; ustar = fill
  frzpot = fill; mltpot = fill; util2 = fill; util3 = fill
  do nt = 1, ntr
    trflx(nt,:,:) = fill
  end do
  do nt = 1, kk+1
    t_rs_nonloc(:,:,nt) = fill; s_rs_nonloc(:,:,nt) = fill
  end do
  call thermf_cesm(m,n,mm,nn,k1m,k1n)
  do nt = 1, ntr
    tf(:,:,nt) = trflx(nt,:,:)
  end do
  open (newunit=u, file='out.bin', access='stream', form='unformatted', status='replace')
  write (u) surflx, sswflx, surrlx, salflx, brnflx, salrlx, hmltfz, ustar, frzpot, mltpot, util2, util3, salt_corr
  write (u) tf, trc_corr, t_rs_nonloc, s_rs_nonloc, tflxdi, sflxdi
  write (u) nflxdi
  close (u)
end program thermf_cesm_driver
