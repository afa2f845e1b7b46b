! constants -- drop-in for the fork's module of the same name (lib/constants.f90): the one named constant its drivers use.
module constants
 implicit none
 double precision,parameter :: pi=3.14159265358979323846d0
end module constants
