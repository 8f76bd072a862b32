// jacobi3.inc — the rotation of the fp64 3x3 cyclic Jacobi eigen-solve, shared by k_gicp_knn_cov (gicp_kernels.hip) and
// k_normals (normal_kernels.hip).  Included inside the kernel file's anonymous namespace.
// one Jacobi rotation of the symmetric 3x3 in the (p, q) plane; r is the third index.  V's columns p, q follow.
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                           double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    double a, b;
    a = c * v0p - s * v0q; b = s * v0p + c * v0q; v0p = a; v0q = b;
    a = c * v1p - s * v1q; b = s * v1p + c * v1q; v1p = a; v1q = b;
    a = c * v2p - s * v2q; b = s * v2p + c * v2q; v2p = a; v2q = b;
}
