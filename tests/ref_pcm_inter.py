"""Float64 numpy reference for the two-graph form of the pairwise consistency test (cgmr_closure_consistency_inter).  TEST
INFRASTRUCTURE ONLY; shares no code with the device.

Candidate k = (a_k, p_k, z_k, Omega_k): a_k an own vertex, p_k the pose of a peer's vertex as the peer sent it, z_k a measurement
of x_a^-1 x_p.  For l < k

    eps_kl = z_k (+) (p_k^-1 (+) p_l) (+) z_l^-1 (+) (x_al^-1 (+) x_ak)

which is ref_pcm's loop with x_b replaced by p, so compose, inverse and the forward-accumulated Jacobians are ref_pcm's, and

    S_kl = J_a Sigma_a J_a^T + J_p Sigma_p J_p^T + J_zk Omega_k^-1 J_zk^T + J_zl Omega_l^-1 J_zl^T

Sigma_a the 6x6 joint covariance of (x_ak, x_al), Sigma_p the 6x6 joint covariance of (p_k, p_l) (zero when the caller has
none: the peer's poses taken as exact)."""
import numpy as np

import ref_joint_marginals as J
import ref_pcm as P


INPUTS = ("ak", "pk", "al", "pl", "zk", "zl")


def loop_residual_inter(xak, pk, xal, pl, zk, zl):
    """The residual written out from its definition (the peer's relative pose, then the own one)."""
    peer = P.compose(P.inverse(pk), pl)
    mine = P.compose(P.inverse(xal), xak)
    return P.compose(P.compose(P.compose(zk, peer), P.inverse(zl)), mine)


def loop_jacobians_inter(xak, pk, xal, pl, zk, zl):
    """(eps, {name: d eps / d input}) for ``INPUTS``: ref_pcm's forward accumulation with p in x_b's place."""
    eps, jac = P.loop_jacobians(xak, pk, xal, pl, zk, zl)
    return eps, {"ak": jac["ak"], "pk": jac["bk"], "al": jac["al"], "pl": jac["bl"], "zk": jac["zk"], "zl": jac["zl"]}


def pair_terms_inter(Sa6, Sp6, xak, pk, xal, pl, zk, zl, info_k, info_l):
    """(eps, S, scale): Sa6 the joint covariance of (x_ak, x_al), Sp6 that of (p_k, p_l) or None; scale = the sum over the
    block terms of both of ||J_i|| ||J_j|| ||Sigma_ij|| (Frobenius), the size of what S is added up from."""
    eps, jac = loop_jacobians_inter(xak, pk, xal, pl, zk, zl)
    Ja = np.hstack([jac["ak"], jac["al"]])
    Jp = np.hstack([jac["pk"], jac["pl"]])
    if Sp6 is None:
        Sp6 = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        S = Ja @ Sa6 @ Ja.T + Jp @ Sp6 @ Jp.T + jac["zk"] @ np.linalg.inv(P.info_full(info_k)) @ jac["zk"].T \
            + jac["zl"] @ np.linalg.inv(P.info_full(info_l)) @ jac["zl"].T
    scale = 0.0
    for names, Sig in ((("ak", "al"), Sa6), (("pk", "pl"), Sp6)):
        for i in range(2):
            for j in range(2):
                scale += np.linalg.norm(jac[names[i]]) * np.linalg.norm(jac[names[j]]) * np.linalg.norm(Sig[3 * i:3 * i + 3, 3 * j:3 * j + 3])
    return eps, S, scale


def pair_d2_inter(Sa6, Sp6, xak, pk, xal, pl, zk, zl, info_k, info_l):
    """eps^T S^-1 eps; NaN where S is not finite or not positive definite."""
    eps, S, _ = pair_terms_inter(Sa6, Sp6, xak, pk, xal, pl, zk, zl, info_k, info_l)
    S = 0.5 * (S + S.T)
    if not np.all(np.isfinite(S)) or np.linalg.eigvalsh(S).min() <= 0:
        return np.nan
    return float(eps @ np.linalg.solve(S, eps))


def gather6(Sq, idx):
    """The 6x6 joint covariance of the two positions ``idx`` out of a joint matrix."""
    rows = np.concatenate([np.arange(3 * i, 3 * i + 3) for i in idx])
    return Sq[np.ix_(rows, rows)]


def unique_own(ca):
    """(unique own vertices in order of first appearance, position of every a)."""
    uq, where = [], {}
    for v in ca:
        if int(v) not in where:
            where[int(v)] = len(uq)
            uq.append(int(v))
    return np.array(uq, dtype=np.int32), [where[int(v)] for v in ca]


def consistency_from_joint_inter(Sq, pos_a, poses, ca, peer_pose, cmeas, cinfo, peer_cov=None):
    """d2 [N, N] from a joint covariance ``Sq`` of some own query list in which candidate k's own end sits at pos_a[k]."""
    N = len(ca)
    d2 = np.zeros((N, N))
    for k in range(N):
        for l in range(k):
            Sp6 = None if peer_cov is None else gather6(peer_cov, (k, l))
            d2[k, l] = d2[l, k] = pair_d2_inter(gather6(Sq, (pos_a[k], pos_a[l])), Sp6, poses[ca[k]], peer_pose[k], poses[ca[l]],
                                                peer_pose[l], cmeas[k], cmeas[l], cinfo[k], cinfo[l])
    return d2


def consistency_dense_inter(poses, fixed, ef, et, meas, info, ca, peer_pose, cmeas, cinfo, peer_cov=None):
    """d2 [N, N], the own covariance from the dense inverse of H (ref_joint_marginals.joint_dense over the unique own ends)."""
    uq, pa = unique_own(ca)
    Sq = J.joint_dense(poses, fixed, ef, et, meas, info, uq)
    f64 = lambda x: np.asarray(x, dtype=np.float64)   # noqa: E731
    return consistency_from_joint_inter(Sq, pa, f64(poses), ca, f64(peer_pose), f64(cmeas), f64(cinfo),
                                        None if peer_cov is None else f64(peer_cov))
