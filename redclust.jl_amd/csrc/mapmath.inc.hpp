// The two elementary functions of the MAP search's scores (mapsearch.inc.hip, phase B), host and device: included by
// redclust_hip.hip in front of mapsearch.inc.hip and, with __host__ and __device__ defined away, by the CPU test that holds them
// against libm (tests/test_mapsearch_cpu.py).  Nothing but <cmath>'s log is needed.

// lgΓ(x) for x > 0 by Stirling's series at y = x + m >= 16 and lgΓ(x) = lgΓ(y) − log(x(x+1)…(y−1)): the next term of the series,
// y^-13/156, is below 2e-18 there, so the error is the rounding of (y − ½)·log y − y: a few ulp of that product.  The device
// library's lgamma and log1p keep coefficient tables live across the visit loop that alone exceed the 256 VGPRs a lane may
// have; this one and log1p_lean below share the constants of one log.
__host__ __device__ inline double lgamma_pos(double x)
{
    double prod = 1.0, y = x;
    while (y < 16.0) { prod *= y; y += 1.0; }
    const double w = 1.0 / (y * y);
    double s = -691.0 / 360360.0;
    s = s * w + 1.0 / 1188.0;
    s = s * w - 1.0 / 1680.0;
    s = s * w + 1.0 / 1260.0;
    s = s * w - 1.0 / 360.0;
    s = s * w + 1.0 / 12.0;
    return ((y - 0.5) * log(y) - y + 0.91893853320467274178) + s / y - (prod != 1.0 ? log(prod) : 0.0);   // (x >= 16: no second log)
}
// log(1 + x) for x > −1 from one log: log(u) with u = fl(1 + x), corrected by the rounding error of u over u
__host__ __device__ inline double log1p_lean(double x)
{
    const double u = 1.0 + x;
    return u == 1.0 ? x : log(u) - ((u - 1.0) - x) / u;
}
