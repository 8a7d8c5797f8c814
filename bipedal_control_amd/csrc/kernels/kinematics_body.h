// The text of the kinematic primitives: kinematics.h includes it twice (fused::, exact::), nothing else does, hence no include guard.  Every function
// does nothing but its expression; operand order and grouping are part of the contract (tests/test_gpu_kinematics_parent_bits.py).
KIN_FN void cross3(const double* a, const double* b, double* c) { KIN_FP
  const double c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
  c[0] = c0; c[1] = c1; c[2] = c2;
}
KIN_FN double dot3(const double* a, const double* b) { KIN_FP
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
KIN_FN void mat3_vec(const double* A, const double* v, double* y) { KIN_FP
  const double y0 = A[0] * v[0] + A[1] * v[1] + A[2] * v[2], y1 = A[3] * v[0] + A[4] * v[1] + A[5] * v[2], y2 = A[6] * v[0] + A[7] * v[1] + A[8] * v[2];
  y[0] = y0; y[1] = y1; y[2] = y2;
}
// C = A B; C may be A or B
KIN_FN void mat3_mul(const double* A, const double* B, double* C) { KIN_FP
  double t[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) t[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
  for (int i = 0; i < 9; ++i) C[i] = t[i];
}
// y = S v for a symmetric 3x3 stored as xx, xy, xz, yy, yz, zz
KIN_FN void sym3_vec(const double* S, const double* v, double* y) { KIN_FP
  const double y0 = S[0] * v[0] + S[1] * v[1] + S[2] * v[2], y1 = S[1] * v[0] + S[3] * v[1] + S[4] * v[2], y2 = S[2] * v[0] + S[4] * v[1] + S[5] * v[2];
  y[0] = y0; y[1] = y1; y[2] = y2;
}

// R = Rz(yaw) Ry(pitch) Rx(roll) from the sines and cosines of the three angles
KIN_FN void rot_zyx(double sy, double cy, double sp, double cp, double sr, double cr, double* R) { KIN_FP
  R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
  R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
  R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
}
// Rodrigues: the rotation about the unit vector `axis` by the angle whose sine and cosine are s, c
KIN_FN void axis_angle(const double* a, double s, double c, double* rot) { KIN_FP
  const double vv = 1.0 - c;
  rot[0] = c + vv * a[0] * a[0];        rot[1] = vv * a[0] * a[1] - s * a[2]; rot[2] = vv * a[0] * a[2] + s * a[1];
  rot[3] = vv * a[1] * a[0] + s * a[2]; rot[4] = c + vv * a[1] * a[1];        rot[5] = vv * a[1] * a[2] - s * a[0];
  rot[6] = vv * a[2] * a[0] - s * a[1]; rot[7] = vv * a[2] * a[1] + s * a[0]; rot[8] = c + vv * a[2] * a[2];
}
// E = Rfix axis_angle(axis, q): the joint-local rotation (oracle/wbc_py.py fk)
KIN_FN void joint_rotation(const double* Rfix, const double* axis, double s, double c, double* E) { KIN_FP
  double rot[9];
  axis_angle(axis, s, c, rot);
  mat3_mul(Rfix, rot, E);
}
// one joint down the chain: o += R pfix, then R = R E
KIN_FN void chain_step(double* R, double* o, const double* pfix, const double* E) { KIN_FP
  double t[3];
  mat3_vec(R, pfix, t);
  for (int i = 0; i < 3; ++i) o[i] += t[i];
  mat3_mul(R, E, R);
}
// pt = o + R off
KIN_FN void point_on_body(const double* R, const double* o, const double* off, double* pt) { KIN_FP
  double t[3];
  mat3_vec(R, off, t);
  for (int i = 0; i < 3; ++i) pt[i] = o[i] + t[i];
}
// Iw = R I R' of a symmetric I, both as xx, xy, xz, yy, yz, zz
KIN_FN void world_inertia(const double* R, const double* I, double* Iw) { KIN_FP
  const double Ib[9] = {I[0], I[1], I[2], I[1], I[3], I[4], I[2], I[4], I[5]};
  double T[9];
  mat3_mul(R, Ib, T);
  Iw[0] = T[0] * R[0] + T[1] * R[1] + T[2] * R[2]; Iw[1] = T[0] * R[3] + T[1] * R[4] + T[2] * R[5]; Iw[2] = T[0] * R[6] + T[1] * R[7] + T[2] * R[8];
  Iw[3] = T[3] * R[3] + T[4] * R[4] + T[5] * R[5]; Iw[4] = T[3] * R[6] + T[4] * R[7] + T[5] * R[8]; Iw[5] = T[6] * R[6] + T[7] * R[7] + T[8] * R[8];
}
// Euler-angle rates (yaw, pitch, roll) from the world angular velocity w: solve E thetadot = w, E = [e_z, Rz e_y, Rz Ry e_x]
KIN_FN void euler_rates_from_world_omega(double sy, double cy, double sp, double cp, const double* w, double* rates) { KIN_FP
  const double rr = (cy * w[0] + sy * w[1]) / cp;      // roll rate
  const double pr = -sy * w[0] + cy * w[1];            // pitch rate
  rates[0] = w[2] + sp * rr; rates[1] = pr; rates[2] = rr;
}
// mode id -> is contact point c in contact (0, 1 left foot; 2, 3 right foot; MotionPhaseDefinition.h:57-76).  A mode outside 0..3 has none
KIN_FN bool stance_flag(int mode, int c) { return c < 2 ? (mode == 1 || mode == 3) : (mode == 2 || mode == 3); }
