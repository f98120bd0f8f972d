!! test_mfp_hip -- `test_mfp` (tests/test_poisson_mf.f90) on the GPU.
!! Same CLI (<grid size> <iterations per restart>), same manufactured problem
!! (b = A*1, tol = 1e-15, Chebyshev params (8.2, 0.2)) and the same printed
!! lines; the only source change a reference user makes is the call names:
!!   stvec -> hip_poisson5, cbpr2 -> hip_cbpr2,
!!   gmres_hh_prec_omp -> gmres_hh_prec_hip, gmres_mgsr_omp -> gmres_mgsr_hip.
!! An optional third argument `right` runs the MGS-R solve alone, preconditioned
!! on the right (side = GK_SIDE_RIGHT: its "Final residual" is the true one); `f32`
!! runs it alone on the compressed basis (basis = GK_BASIS_F32: the Krylov columns
!! stored as FP32); `cgs2` runs it alone with the CGS2 Arnoldi step (orth = GK_ORTH_CGS2);
!! `hhright` runs the Householder solve alone, preconditioned on the
!! right (gmres_hh_prec_hip(..., side = GK_SIDE_RIGHT)), and prints its final residual
!! a second time with every digit; `mg` runs the MGS-R solve alone with the multigrid
!! V-cycle hip_mg on the right (smoother interval (8, 1), tol 1e-12), then pcg_hip with it;
!! `shift` runs those two legs on the shifted operator A + 0.5 I (hip_set_shift(0.5):
!! b = (A + 0.5 I)*1 through hip_poisson5, smoother interval (8.5, 1.5)).
program test_mfp_hip
    use gmres_hip
    implicit none
    integer :: nsize, max_iter, n_args
    character(len=32) :: arg_str
    logical :: right, f32, hhright, cgs2, mg, shifted
    n_args = command_argument_count()
    if (n_args < 2) then
        print *, "usage ./test_mfp_hip <grid size> <iterations per restart> [right|f32|cgs2|shift|hhright|mg]"
        stop
    end if
    right = .false.; f32 = .false.; hhright = .false.; cgs2 = .false.; mg = .false.; shifted = .false.
    if (n_args >= 3) then
        call get_command_argument(3, arg_str)
        right = trim(arg_str) == 'right'
        f32 = trim(arg_str) == 'f32'
        cgs2 = trim(arg_str) == 'cgs2'
        hhright = trim(arg_str) == 'hhright'
        shifted = trim(arg_str) == 'shift'
        mg = trim(arg_str) == 'mg' .or. shifted
    end if
    if (shifted) call hip_set_shift(0.5d0)
    call get_command_argument(1, arg_str)
    read (arg_str, *) nsize
    call get_command_argument(2, arg_str)
    read (arg_str, *) max_iter
    write (*, '(60("-"))')
    if (.not. right .and. .not. f32 .and. .not. cgs2 .and. .not. mg) then
        call run(nsize, max_iter, .true.)
        write (*, '(60("-"))')
    end if
    if (.not. hhright) then
        call run(nsize, max_iter, .false.)
        write (*, '(60("-"))')
    end if
    if (mg) then
        call run_pcg_mg(nsize)
        write (*, '(60("-"))')
    end if
    call hip_release()
contains
    subroutine run_pcg_mg(nsize)
        integer, intent(in) :: nsize
        real(8), allocatable :: b(:), x(:)
        real(8) :: params(2), res
        integer :: iter
        allocate (b(nsize*nsize), x(nsize*nsize))
        params = [8.0d0, 1.0d0]
        if (shifted) params = [8.5d0, 1.5d0]
        x = 1.0d0
        call hip_poisson5(x, b, nsize)
        iter = 200
        if (shifted) then
            write (*, '(A)') 'PCG Poisson 2D Test Matrix Free (shifted A + 0.5 I, multigrid V-cycle, MI355X)'
        else
            write (*, '(A)') 'PCG Poisson 2D Test Matrix Free (multigrid V-cycle, MI355X)'
        end if
        call pcg_hip(hip_poisson5, b, x, 1.d-10, iter, res, hip_mg, params)
        write (*, '(A30, I8)') 'PCG iterations:', iter
        write (*, '(A30, ES12.4)') 'PCG residual:', res
        write (*, '(A30, ES12.4)') 'PCG max error L_max:', maxval(abs(x - 1.0d0))
    end subroutine run_pcg_mg

    subroutine run(nsize, max_iter, householder)
        integer, intent(in) :: nsize, max_iter
        logical, intent(in) :: householder
        real(8), allocatable :: b(:), x(:), errn(:), verr(:), params(:)
        real(8) :: tol
        integer :: n_iter, n_stages, c0, c1, crate
        tol = 1.d-15
        allocate (b(nsize*nsize), x(nsize*nsize), params(2))
        params(1) = 8.2d0; params(2) = 0.2d0
        if (mg) then
            tol = 1.d-12
            params(1) = 8.0d0; params(2) = 1.0d0
            if (shifted) then
                params(1) = 8.5d0; params(2) = 1.5d0
            end if
        end if
        x = 1.0d0
        call hip_poisson5(x, b, nsize)   ! b = A*1: every solution entry must be 1.0
        if (householder .and. hhright) then
            write (*, '(A)') 'GMRES Poisson 2D Test Matrix Free (Householder Chebyshev on the right, MI355X)'
        else if (householder) then
            write (*, '(A)') 'GMRES Poisson 2D Test Matrix Free (Householder Chebyshev, MI355X)'
        else if (right) then
            write (*, '(A)') 'GMRES Poisson 2D Test Matrix Free (MGSR Chebyshev on the right, MI355X)'
        else if (f32) then
            write (*, '(A)') 'GMRES Poisson 2D Test Matrix Free (MGSR Chebyshev, compressed basis, MI355X)'
        else if (cgs2) then
            write (*, '(A)') 'GMRES Poisson 2D Test Matrix Free (CGS2 Chebyshev, MI355X)'
        else if (shifted) then
            write (*, '(A)') 'GMRES Poisson 2D Test Matrix Free (shifted A + 0.5 I, MGSR multigrid V-cycle on the right, MI355X)'
        else if (mg) then
            write (*, '(A)') 'GMRES Poisson 2D Test Matrix Free (MGSR multigrid V-cycle on the right, MI355X)'
        else
            write (*, '(A)') 'GMRES Poisson 2D Test Matrix Free (MGSR Chebyshev, MI355X)'
        end if
        write (*, '(A,I8,A18,I5,A8,ES10.2)') "N VARS=", nsize*nsize, " MAX ITERS/STAGE=", max_iter, " TOL=", tol
        call system_clock(c0, crate)
        if (householder .and. hhright) then
            call gmres_hh_prec_hip(hip_poisson5, b, x, max_iter, tol, errn, verr, n_iter, n_stages, hip_cbpr2, params, &
                                   side=GK_SIDE_RIGHT)
        else if (householder) then
            call gmres_hh_prec_hip(hip_poisson5, b, x, max_iter, tol, errn, verr, n_iter, n_stages, hip_cbpr2, params)
        else if (right) then
            call gmres_mgsr_hip(hip_poisson5, b, x, max_iter, tol, errn, verr, n_iter, n_stages, hip_cbpr2, params, &
                                side=GK_SIDE_RIGHT)
        else if (f32) then
            call gmres_mgsr_hip(hip_poisson5, b, x, max_iter, tol, errn, verr, n_iter, n_stages, hip_cbpr2, params, &
                                basis=GK_BASIS_F32)
        else if (cgs2) then
            call gmres_mgsr_hip(hip_poisson5, b, x, max_iter, tol, errn, verr, n_iter, n_stages, hip_cbpr2, params, &
                                orth=GK_ORTH_CGS2)
        else if (mg) then
            call gmres_mgsr_hip(hip_poisson5, b, x, max_iter, tol, errn, verr, n_iter, n_stages, hip_mg, params, &
                                side=GK_SIDE_RIGHT)
        else
            call gmres_mgsr_hip(hip_poisson5, b, x, max_iter, tol, errn, verr, n_iter, n_stages, hip_cbpr2, params)
        end if
        call system_clock(c1)
        write (*, '(A30, I8, A10, I4)') 'Iterations until convergence:', (n_stages - 1)*max_iter + n_iter, &
            ' Stages=', n_stages
        write (*, '(A30, ES12.4)') "Final ||I - V.t * V||:", verr(n_iter)
        write (*, '(A30, ES12.4)') 'Final residual:', errn(n_iter)
        if (hhright) write (*, '(A30, ES24.16)') 'Final residual, every digit:', errn(n_iter)
        write (*, '(A30, ES12.4)') 'Max error L_max:', maxval(abs(x - 1.0d0))
        write (*, '(A30, ES12.4)') 'L2 norm:', norm2(x - 1.0d0)
        write (*, '(A30, 10F10.4)') 'First 10 solution elements', x(1:10)
        write (*, '(A30, F12.4, A)') 'Elapsed time:', dble(c1 - c0)/dble(crate), ' secs.'
    end subroutine run
end program test_mfp_hip
