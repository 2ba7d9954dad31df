"""The mirrored-pairs case of the symmetry tests, shared by the host test (the
oracle's control step) and the GPU test (k_step): 4 airborne Go2 envs as two mirrored pairs, env
2k + 1 starting from the mirror image of env 2k's root and joint state and receiving mirrored
commands and actions for 4 control steps.

The state is chosen so that a wrong table cannot pass.  A joint's velocity decays within one
control step under the task's PD gains (kd / kp = 25 ms), so the PD targets ramp at a constant
joint speed v and the joints start in the ramp's steady state (q = target - v kd / kp): the
velocities stay near v for all 4 steps.  Speeds, actions and base rates are picked so that on
every row of env 2k each entry mirrored with sign -1 is at least 0.1 in magnitude and paired
entries differ by at least 0.1 (`separation`, asserted by both tests): one wrong sign or one
swapped pair then misses BOUND by more than two orders of magnitude.
"""
import numpy as np

F = np.float32
STEPS, N = 4, 4
# The largest |obs_B - mirror(obs_A)| the CPU oracle itself shows on this case over the 4 steps
# (fp32 rounding of mirrored operation orders, amplified by the dynamics): measured 1.292e-4
# (per step: 6.46e-5, 8.77e-5, 1.292e-4, 1.248e-4).
ORACLE_DEVIATION = 1.292e-4
BOUND = 4 * ORACLE_DEVIATION
SEPARATION = 0.1

# per pair: the first step's actions and the ramp's joint speeds, DOF order FL, FR, RL, RR x (hip, thigh, calf)
ACT = 1.5 * np.array([[0.8, -1.2, 1.6, 1.3, 0.7, -0.9, -1.1, 1.9, -0.6, 0.5, -1.4, 1.3],
                      [-1.0, 0.6, -1.7, -0.4, -1.3, 1.1, 0.9, -0.7, 1.2, 1.8, 1.6, -0.5]], F)
SPEED = np.sign(ACT) * np.array([[3.2, 5.5, 2.6, 6.0, 2.5, 5.6, 6.2, 2.8, 6.2, 3.2, 5.9, 3.1],
                                 [6.0, 2.9, 6.1, 3.2, 6.0, 3.0, 6.2, 5.6, 3.2, 3.2, 2.5, 5.9]], F)
COMMANDS = np.array([[0.9, -0.5, 0.7, 0.0], [-0.6, 0.8, -1.1, 0.0]], F)


def cfg_edit(cfg):
    """Noise, pushes, every randomisation and command resampling off."""
    cfg.noise.add_noise = False
    dr = cfg.domain_rand
    dr.push_robots = dr.randomize_friction = dr.randomize_base_mass = False
    for s in ("randomize_kp", "randomize_kd", "randomize_motor_strength", "randomize_action_delay"):
        setattr(dr, s, False)
    cfg.commands.heading_command = False
    cfg.commands.resampling_time = 1000.0


def mirror(x, table):
    perm, sign = table
    return (np.asarray(sign, F) * np.asarray(x, F)[..., np.asarray(perm)]).astype(F)


def _quat(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy])


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def initial_state(default_dof_pos, joints, kp=20.0, kd=0.5, action_scale=0.25):
    """(root [4, 13], dof pos [4, D], dof vel [4, D]): env 2k from the constants above, env 2k + 1
    its mirror image: position (x, -y, z), quaternion (-qx, qy, -qz, qw), linear velocity (+,-,+),
    angular velocity (-,+,-), joints through the joint table."""
    d = np.asarray(default_dof_pos, np.float64).reshape(-1)
    root, q, qd = np.zeros((N, 13), F), np.zeros((N, len(d)), F), np.zeros((N, len(d)), F)
    for k in range(2):
        a = 2 * k
        root[a, :3] = [0.3 + k, 0.7 - k, 3.0]
        root[a, 3:7] = _quat(0.5 - 1.0 * k, 0.35, 0.6 + k)
        R = _rot(root[a, 3:7].astype(np.float64))
        root[a, 7:10] = R @ np.array([0.8, -0.6 + 1.3 * k, 0.4])      # given in the base frame,
        root[a, 10:13] = R @ np.array([2.4 - 4.8 * k, -3.0, 2.0 - 4.2 * k])  # which the rows show
        q[a] = d + action_scale * ACT[k] - SPEED[k] * kd / kp
        qd[a] = SPEED[k]
        root[a + 1, :3] = root[a, :3] * [1, -1, 1]
        root[a + 1, 3:7] = root[a, 3:7] * [-1, 1, -1, 1]
        root[a + 1, 7:10] = root[a, 7:10] * [1, -1, 1]
        root[a + 1, 10:13] = root[a, 10:13] * [-1, 1, -1]
        q[a + 1], qd[a + 1] = mirror(q[a], joints), mirror(qd[a], joints)
    return root, q, qd


def step_inputs(step, joints, dt=0.02, action_scale=0.25):
    """(actions [4, D], commands [4, 4]) of control step `step`: the ramping targets, mirrored."""
    act, cmd = np.zeros((N, ACT.shape[1]), F), np.zeros((N, 4), F)
    for k in range(2):
        a = 2 * k
        act[a] = ACT[k] + SPEED[k] * F(dt / action_scale) * (step + 1)
        act[a + 1] = mirror(act[a], joints)
        cmd[a] = COMMANDS[k]
        cmd[a + 1] = COMMANDS[k] * [1, -1, -1, 1]
    return act, cmd


def separation(row, table):
    """The smallest of: |entry| over the entries the table mirrors with sign -1, and
    |entry - partner| over the entries it moves."""
    perm, sign = np.asarray(table[0]), np.asarray(table[1])
    row = np.asarray(row, F)
    neg, moved = sign < 0, perm != np.arange(len(perm))
    return min(np.abs(row[perm][neg]).min(), np.abs(row - row[perm])[moved].min())


def deviation(rows, table):
    """max |row_B - mirror(row_A)| over the two pairs."""
    return max(float(np.abs(rows[a + 1] - mirror(rows[a], table)).max()) for a in (0, 2))
