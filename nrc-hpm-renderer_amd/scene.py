"""Host-side scene inputs of the NRC-HPM path (values only; no Vulkan plumbing).

Mirrors what the reference uploads as UBOs/textures before a frame:
  * camera          src/Camera.cpp:164-174 (glm::perspective * glm::lookAt, inverse), defaults src/main.cu:180-187
  * scene presets   src/AppConfig.cpp:93-150 (HpmSceneConfig ids 0-5)
  * lights          src/HpmScene.cpp:28-30, src/DirLight.cpp:5-14
  * volume box      src/NrcHpmRenderer.cu:910-912 (normalize(extent) * 107.5), g = 0.8 src/HpmScene.cpp:45
  * density texel   src/Texture3D.cpp:106 (uint8(v*255) truncation), stored here as ONE channel (R8)
Synthetic volumes / env map follow SURVEY.md section 8(d) (seeded, deterministic).
"""
import math

import numpy as np

SCENE_PRESETS = {  # id: (dirLightStrength, pointLightStrength, hdrEnvMapStrength, density)
    0: (16.0, 0.0, 0.0, 0.6),
    1: (0.0, 64.0, 0.0, 0.6),
    2: (0.0, 128.0, 0.0, 1.0),
    3: (16.0, 0.0, 0.0, 0.25),
    4: (8.0, 0.0, 0.1, 0.6),
    5: (0.0, 0.0, 1.0, 1.6),
}


def perspective(fovy, aspect, near, far):
    """glm::perspective, GL clip space (depth -1..1), right handed."""
    t = math.tan(fovy / 2.0)
    m = np.zeros((4, 4), np.float64)
    m[0, 0] = 1.0 / (aspect * t)
    m[1, 1] = 1.0 / t
    m[2, 2] = -(far + near) / (far - near)
    m[3, 2] = -1.0
    m[2, 3] = -(2.0 * far * near) / (far - near)
    return m


def look_at(eye, center, up):
    eye, center, up = (np.asarray(v, np.float64) for v in (eye, center, up))
    f = center - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[0, 3], m[1, 3], m[2, 3] = -s.dot(eye), -u.dot(eye), f.dot(eye)
    return m


def make_camera(pos=(64.0, 0.0, 0.0), view_dir=(-1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), aspect=1920.0 / 1080.0,
                fovy=math.radians(60.0), near=0.1, far=100.0):
    """CameraMatrices.invProjView (column-major, as glm stores it) + camera.pos."""
    pos = np.asarray(pos, np.float64)
    pv = perspective(fovy, aspect, near, far) @ look_at(pos, pos + np.asarray(view_dir, np.float64), up)
    inv = np.linalg.inv(pv)
    return dict(inv_proj_view=np.ascontiguousarray(inv.T.astype(np.float32).reshape(16)),  # column-major
                pos=pos.astype(np.float32))


def orbit_cameras(n, radius=64.0, height=0.0, aspect=1920.0 / 1080.0, center=(0.0, 0.0, 0.0), start_angle=0.0, **camera_kw):
    """A turntable: n make_camera views on the circle of `radius` around `center` (the volume's centre: the box is centred on the origin)
    in the plane y = center.y + height, every one looking at `center`.  View k stands at angle start_angle + 2 pi k / n from the x axis
    towards z, so view 0 of the defaults is make_camera's default view.  camera_kw goes to make_camera (up, fovy, near, far).
    What NrcHpmRenderer.RenderPath / McHpmRenderer.RenderPath take."""
    n = int(n)
    if n < 1:
        raise ValueError("orbit_cameras: n must be at least 1")
    if not (radius > 0.0 or height != 0.0):
        raise ValueError("orbit_cameras: the eye must not stand on the centre (radius > 0 or height != 0)")
    c = np.asarray(center, np.float64)
    cams = []
    for k in range(n):
        a = start_angle + 2.0 * math.pi * k / n
        pos = c + np.array([radius * math.cos(a), height, radius * math.sin(a)], np.float64)
        cams.append(make_camera(pos=pos, view_dir=c - pos, aspect=aspect, **camera_kw))
    return cams


def dir_light_dir(zenith=-1.57, azimuth=0.0):
    """VecFromAngles (src/DirLight.cpp:5-14): Ry(azimuth) * Rx(zenith) * (0,1,0)."""
    cz, sz = math.cos(zenith), math.sin(zenith)
    v = np.array([0.0, cz, sz])
    ca, sa = math.cos(azimuth), math.sin(azimuth)
    return np.array([ca * v[0] + sa * v[2], v[1], -sa * v[0] + ca * v[2]], np.float32)


def volume_size(dims):
    """skySize = normalize(vec3(extent)) * 107.5 in fp32 (src/NrcHpmRenderer.cu:910-912)."""
    d = np.asarray(dims, np.float32)
    n = np.float32(np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1]) + np.float32(d[2] * d[2])))
    return (d / n * np.float32(107.5)).astype(np.float32)


def quantize_density(vol_f32):
    """src/Texture3D.cpp:106: uint8(value * 255.0f) (truncation). Input indexed [i][j][k] = (x,y,z)."""
    q = (np.asarray(vol_f32, np.float32) * np.float32(255.0)).astype(np.uint8)
    # memory order of the texture: index = i + W*j + W*H*k  -> array [k][j][i]
    return np.ascontiguousarray(q.transpose(2, 1, 0))


def volume_to_bricks(vol):
    """A dense [nz][ny][nx] uint8 or float32 volume as the brick list of SetVolumeBricks (include/nrc_hpm.h, nrc_renderer_set_volume_bricks):
    (origins int32 [n][3] = (x0, y0, z0), bricks [n][8][8][8] = [dz][dy][dx]) of the aligned 8^3 cells that hold a non-zero voxel, in
    cell order z, y, x; cells at the volume's edge are padded with zeros."""
    vol = np.asarray(vol)
    if vol.ndim != 3 or vol.dtype not in (np.uint8, np.float32):
        raise ValueError("volume_to_bricks: a [nz][ny][nx] uint8 or float32 array (got %s %s)" % (vol.dtype, vol.shape))
    nz, ny, nx = vol.shape
    gz, gy, gx = (nz + 7) // 8, (ny + 7) // 8, (nx + 7) // 8
    padded = np.zeros((gz * 8, gy * 8, gx * 8), vol.dtype)
    padded[:nz, :ny, :nx] = vol
    cells = padded.reshape(gz, 8, gy, 8, gx, 8).transpose(0, 2, 4, 1, 3, 5)      # [cz][cy][cx][dz][dy][dx]
    cz, cy, cx = np.nonzero((cells != 0).any(axis=(3, 4, 5)))
    origins = (np.stack([cx, cy, cz], axis=1) * 8).astype(np.int32).reshape(-1, 3)
    return np.ascontiguousarray(origins), np.ascontiguousarray(cells[cz, cy, cx]).reshape(-1, 8, 8, 8)


def bricks_to_volume(origins, bricks, dims, ignore_invalid=False):
    """The dense volume a brick list stands for, dims = its shape (nz, ny, nx): the inverse of volume_to_bricks and the CPU statement of
    SetVolumeBricks.  Voxels no brick covers are 0, brick voxels past the edge are dropped, of several bricks with one origin the last
    wins.  An origin that is not a multiple of 8 inside the volume raises ValueError (what the call does with a host list) or, with
    ignore_invalid, is skipped (what the kernels do with a device list)."""
    origins, bricks = np.asarray(origins), np.asarray(bricks)
    n = origins.shape[0]
    if origins.shape != (n, 3) or bricks.shape != (n, 8, 8, 8):
        raise ValueError("bricks_to_volume: origins [n][3] and bricks [n][8][8][8] (got %s and %s)" % (origins.shape, bricks.shape))
    nz, ny, nx = (int(v) for v in dims)
    vol = np.zeros((nz, ny, nx), bricks.dtype)
    for i in range(n):
        x0, y0, z0 = (int(v) for v in origins[i])
        if min(x0, y0, z0) < 0 or x0 % 8 or y0 % 8 or z0 % 8 or x0 >= nx or y0 >= ny or z0 >= nz:
            if ignore_invalid:
                continue
            raise ValueError("bricks_to_volume: brick %d has origin (%d, %d, %d): multiples of 8 inside %dx%dx%d" % (i, x0, y0, z0, nx, ny, nz))
        ez, ey, ex = min(8, nz - z0), min(8, ny - y0), min(8, nx - x0)
        vol[z0:z0 + ez, y0:y0 + ey, x0:x0 + ex] = bricks[i, :ez, :ey, :ex]
    return vol


def key_of_time(t, n_keys):
    """Volume keyframes (include/nrc_hpm.h, nrc_renderer_set_volume_keys): key i sits at time i.  Returns (i, W) of time t -- the in-between
    is made of keys i and i + 1 with weight W / 256 on the latter -- with the library's fp32 roundings: i = min(int(t), n_keys - 1),
    w = t - i, W = int(w * 256 + 0.5), so 0 <= W <= 256 and W = 0 at the last key.  ValueError unless t (as fp32) is finite and inside
    [0, n_keys - 1]."""
    n_keys = int(n_keys)
    t32 = np.float32(t)
    if n_keys < 1 or not np.isfinite(t32) or t32 < np.float32(0.0) or t32 > np.float32(n_keys - 1):
        raise ValueError("key_of_time: time %r is not inside [0, %d] (%d keys)" % (t, n_keys - 1, n_keys))
    i = min(int(t32), n_keys - 1)
    w = np.float32(t32 - np.float32(i))
    return i, int(np.float32(np.float32(w * np.float32(256.0)) + np.float32(0.5)))


def lerp_volume(a, b, W):
    """The in-between of two uint8 volumes, in integers: (a * (256 - W) + b * W + 128) >> 8 per voxel, 0 <= W <= 256 (0: a, 256: b)."""
    W = int(W)
    if not 0 <= W <= 256:
        raise ValueError("lerp_volume: W must be inside [0, 256] (got %d)" % W)
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.shape != b.shape:
        raise ValueError("lerp_volume: two uint8 arrays of one shape (got %s %s and %s %s)" % (a.dtype, a.shape, b.dtype, b.shape))
    return ((a.astype(np.uint32) * np.uint32(256 - W) + b.astype(np.uint32) * np.uint32(W) + np.uint32(128)) >> np.uint32(8)).astype(np.uint8)


def volume_at(keys, t):
    """The CPU statement of SetVolumeTime: the uint8 volume at time t of the key sequence keys[n_keys][nz][ny][nx] (uint8)."""
    keys = np.asarray(keys)
    if keys.ndim != 4 or keys.dtype != np.uint8:
        raise ValueError("volume_at: keys uint8 [n_keys][nz][ny][nx] (got %s %s)" % (keys.dtype, keys.shape))
    i, W = key_of_time(t, keys.shape[0])
    return np.ascontiguousarray(keys[i]) if W == 0 else lerp_volume(keys[i], keys[i + 1], W)


def volumes_to_key_bricks(keys):
    """Dense keys [n_keys][nz][ny][nx] (uint8 or float32, or a sequence of such volumes of one shape) as the arguments of SetVolumeKeyBricks
    (include/nrc_hpm.h, nrc_renderer_set_volume_key_bricks): (counts uint32 [n_keys], origins int32 [sum][3], bricks [sum][8][8][8]) --
    every key's volume_to_bricks list, concatenated in key order."""
    lists = [volume_to_bricks(k) for k in keys]
    if not lists:
        raise ValueError("volumes_to_key_bricks: at least one key")
    if len({np.asarray(k).shape for k in keys}) != 1 or len({b.dtype for _, b in lists}) != 1:
        raise ValueError("volumes_to_key_bricks: keys of one shape and one type")
    counts = np.array([o.shape[0] for o, _ in lists], np.uint32)
    return counts, np.ascontiguousarray(np.concatenate([o for o, _ in lists])), np.ascontiguousarray(np.concatenate([b for _, b in lists]))


def key_bricks_to_volumes(counts, origins, bricks, dims, ignore_invalid=False):
    """The dense keys [n_keys][nz][ny][nx] a brick key sequence stands for, dims = (nz, ny, nx): bricks_to_volume of every key's slice (the
    inverse of volumes_to_key_bricks and the CPU statement of SetVolumeKeyBricks)."""
    counts = [int(c) for c in counts]
    origins, bricks = np.asarray(origins), np.asarray(bricks)
    if sum(counts) != origins.shape[0] or origins.shape[0] != bricks.shape[0]:
        raise ValueError("key_bricks_to_volumes: counts sum to %d, origins hold %d and bricks %d" % (sum(counts), origins.shape[0], bricks.shape[0]))
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    vols = [bricks_to_volume(origins[a:b], bricks[a:b], dims, ignore_invalid) for a, b in zip(first[:-1], first[1:])]
    return np.ascontiguousarray(np.stack(vols)) if vols else np.zeros((0,) + tuple(int(v) for v in dims), bricks.dtype)


def key_brick_bytes(counts, dims):
    """The device bytes a brick key sequence holds (nrc_renderer_volume_key_bytes): 512 * sum(counts) + 4 * n_keys * cells, dims = (nz, ny, nx)"""
    cells = 1
    for n in dims:
        cells *= (int(n) + 7) // 8
    return 512 * sum(int(c) for c in counts) + 4 * len(counts) * cells


def white_env(value=1.0):
    """Quirk Q9 (src/read_file.cpp:129-130): every loaded env texel is overwritten with 1.0."""
    return np.full((1, 1, 4), value, np.float32)


def black_env():
    """Empty hdrEnvMapPath -> 1x1 black (src/read_file.cpp:85-90)."""
    return np.zeros((1, 1, 4), np.float32)


def procedural_sky(w=512, h=256):
    """Synthetic HDR lat-long env map: vertical gradient + sun lobe."""
    v = (np.arange(h, dtype=np.float32) + 0.5) / h
    u = (np.arange(w, dtype=np.float32) + 0.5) / w
    theta = (v - 0.5) * np.float32(math.pi)          # asin(y) range
    phi = (u - 0.5) * np.float32(2 * math.pi)        # atan(z, x) range
    y = np.sin(theta)[:, None] * np.ones((1, w), np.float32)
    x = np.cos(theta)[:, None] * np.cos(phi)[None, :]
    z = np.cos(theta)[:, None] * np.sin(phi)[None, :]
    up = np.clip(y * 0.5 + 0.5, 0, 1)
    sky = (0.25 + 0.75 * up)[..., None] * np.array([0.55, 0.75, 1.0], np.float32)
    sun_dir = np.array([0.0, 0.5, 0.8660254], np.float32)
    c = np.clip(x * sun_dir[0] + y * sun_dir[1] + z * sun_dir[2], 0, 1)
    sun = (c ** 256)[..., None] * np.array([40.0, 36.0, 30.0], np.float32) + (c ** 8)[..., None] * 0.6
    env = np.concatenate([sky + sun, np.ones((h, w, 1), np.float32)], axis=2)
    return np.ascontiguousarray(env.astype(np.float32))


def sphere_volume(n=64):
    """C1 plumbing volume: d(p) = clamp(1 - |p-c|/r, 0, 1), r = 0.45 n."""
    g = (np.arange(n, dtype=np.float32) + 0.5) - n / 2.0
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    d = 1.0 - np.sqrt(x * x + y * y + z * z) / np.float32(0.45 * n)
    d = np.clip(d, 0, 1).astype(np.float32)
    d /= d.max()
    return d


def _value_noise3(n, cells, rng):
    """Trilinear value noise on an n^3 grid from a (cells+1)^3 random lattice."""
    lat = rng.random((cells + 1,) * 3, dtype=np.float32)
    t = np.linspace(0, cells, n, endpoint=False, dtype=np.float32)
    i0 = np.floor(t).astype(np.int32)
    f = t - i0
    f = f * f * (3 - 2 * f)
    i1 = np.minimum(i0 + 1, cells)

    def ax(a, i, axis):
        return np.take(a, i, axis=axis)

    fx, fy, fz = f[:, None, None], f[None, :, None], f[None, None, :]
    c = 0
    for dx, wx in ((i0, 1 - fx), (i1, fx)):
        a = ax(lat, dx, 0)
        for dy, wy in ((i0, 1 - fy), (i1, fy)):
            b = ax(a, dy, 1)
            for dz, wz in ((i0, 1 - fz), (i1, fz)):
                c = c + ax(b, dz, 2) * (wx * wy * wz)
    return c.astype(np.float32)


def fbm_cloud_volume(n=256, seed=1337, octaves=5):
    """C2/C3 cloud: fBm-perturbed ellipsoid, max normalised to exactly 1.0 (src/Texture3D.cpp:74)."""
    rng = np.random.default_rng(seed)
    noise = np.zeros((n, n, n), np.float32)
    amp, cells, tot = 1.0, 4, 0.0
    for _ in range(octaves):
        noise += amp * _value_noise3(n, cells, rng)
        tot += amp
        amp *= 0.5
        cells *= 2
    noise /= tot
    g = (np.arange(n, dtype=np.float32) + 0.5) / n * 2 - 1
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    r = np.sqrt((x / 0.85) ** 2 + (y / 0.6) ** 2 + (z / 0.8) ** 2)
    d = np.clip((1.0 - r) * 1.6 + (noise - 0.5) * 1.8, 0, None)
    d = np.clip(d * 2.5, 0, 1).astype(np.float32)
    d /= d.max()
    return d


def smoke_volume(n=512, seed=1337):
    """C5 heterogeneous smoke plume (seeded)."""
    rng = np.random.default_rng(seed)
    noise = np.zeros((n, n, n), np.float32)
    amp, cells, tot = 1.0, 4, 0.0
    for _ in range(4):
        noise += amp * _value_noise3(n, cells, rng)
        tot += amp
        amp *= 0.5
        cells *= 2
    noise /= tot
    g = (np.arange(n, dtype=np.float32) + 0.5) / n * 2 - 1
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    hgt = (y + 1) * 0.5
    rad = np.sqrt((x - 0.3 * np.sin(4 * hgt)) ** 2 + z ** 2)
    d = np.clip((0.15 + 0.5 * hgt - rad) * 3.0, 0, None) * np.clip(noise * 2.2 - 0.6, 0, None)
    d = np.clip(d, 0, 1).astype(np.float32)
    d /= d.max()
    return d


def cached_volume(kind, n, seed=1337, cache_dir="/tmp"):
    """quantised synthetic volume (`kind`: "cloud" = fbm_cloud_volume, "smoke" = smoke_volume, "sphere"), generated once per
    box and kept as an .npy under `cache_dir` (the 512^3 smoke takes about a minute and 5 GB of host memory to generate)"""
    import os
    gen = {"cloud": fbm_cloud_volume, "smoke": smoke_volume, "sphere": lambda n, seed=0: sphere_volume(n)}[kind]
    path = os.path.join(cache_dir, "nrc_%s_%d_%d.npy" % (kind, n, seed))
    if os.path.exists(path):
        return np.load(path)
    vol = quantize_density(gen(n, seed=seed))
    try:
        tmp = "%s.%d.tmp.npy" % (path, os.getpid())
        np.save(tmp, vol)
        os.replace(tmp, path)
    except OSError:
        pass
    return vol


def make_scene(density_u8, scene_id=4, env=None, g=0.8, dims=None, size=None):
    """Bundle scene inputs.  density_u8: uint8 array in texture memory order [k][j][i] (see quantize_density)."""
    dl, pl, env_s, rho = SCENE_PRESETS[scene_id]
    density_u8 = np.ascontiguousarray(density_u8, np.uint8)
    if dims is None:
        nz, ny, nx = density_u8.shape
        dims = (nx, ny, nz)
    if env is None:
        env = white_env() if env_s != 0.0 else black_env()
    return dict(
        density=density_u8, dims=tuple(int(d) for d in dims),
        size=np.asarray(size if size is not None else volume_size(dims), np.float32),
        density_factor=float(np.float32(rho)), g=float(np.float32(g)),
        dir_light_dir=dir_light_dir(), dir_light_strength=float(dl),
        point_light_pos=np.zeros(3, np.float32), point_light_strength=float(pl),
        point_light_color=np.ones(3, np.float32),
        env=np.ascontiguousarray(env, np.float32), env_strength=float(np.float32(env_s)),
        scene_id=scene_id,
    )


class HpmScene:
    """Host mirror of en::HpmScene (src/HpmScene.cpp:22-100): scene preset + the directional light's angles, with the
    reference's per-frame `Update(deltaTime)`.  Only preset 3 moves when `dynamic` is set (its directional light's azimuth
    advances by deltaTime/2, wrapped at 2*3.141 -- the literal of src/HpmScene.cpp:68); the reference ships every preset with
    dynamic = false (src/AppConfig.cpp:96-150), so this is off unless asked for.  `scene` is the dict make_scene returns;
    hand it to `NrcHpmRenderer.SetSceneParams` / `McHpmRenderer.SetSceneParams` after an update."""

    def __init__(self, density_u8, scene_id=4, env=None, dynamic=False, **kw):
        self.scene = make_scene(density_u8, scene_id=scene_id, env=env, **kw)
        self.scene_id = scene_id
        self.dynamic = bool(dynamic)
        self.zenith, self.azimuth = -1.57, 0.0       # src/HpmScene.cpp:28

    def IsDynamic(self):
        return self.dynamic

    def SetDirLightAngles(self, zenith, azimuth):
        self.zenith, self.azimuth = float(zenith), float(azimuth)
        self.scene["dir_light_dir"] = dir_light_dir(self.zenith, self.azimuth)

    def Update(self, delta_time):
        """returns True when a scene parameter changed"""
        if not self.dynamic or self.scene_id != 3:
            return False
        self.SetDirLightAngles(self.zenith, math.fmod(self.azimuth + delta_time * 0.5, 2.0 * 3.141))
        return True


def light_view(scene, w, h, light_dir=None, margin=1.0):
    """The orthographic view {origin, du, dv, dir} (fp32; api.OrthoAov, api.ortho_rays) of the scene's directional light: the medium's
    shadow map.  Rays travel the way the light does, l = normalize(light_dir or the scene's dir_light_dir) in fp64 (the shadow rays of a
    frame walk the other way, towards -l), across the square spanned by a = normalize(l x (0,1,0)) -- l x (1,0,0) when |l_y| > 0.9 -- and
    b = l x a, of half-width rad = |size| / 2 * margin: the box's bounding sphere at margin 1.  origin = -rad (l + a + b), du = 2 rad a,
    dv = 2 rad b; dir has length 1, so depths are distances from the plane the rays start on.  w, h are the image's size: the view does not
    depend on them."""
    if int(w) <= 0 or int(h) <= 0:
        raise ValueError("light_view: the image size must be positive")
    s = scene.scene if hasattr(scene, "scene") else scene
    l = np.asarray(s["dir_light_dir"] if light_dir is None else light_dir, np.float64).reshape(3)
    n = np.linalg.norm(l)
    if not np.isfinite(n) or n == 0.0:
        raise ValueError("light_view: the light direction must be finite and non-zero")
    l = l / n
    a = np.cross(l, (1.0, 0.0, 0.0) if abs(l[1]) > 0.9 else (0.0, 1.0, 0.0))
    a /= np.linalg.norm(a)
    b = np.cross(l, a)
    rad = 0.5 * float(np.linalg.norm(np.asarray(s["size"], np.float64))) * float(margin)
    return dict(origin=(-rad * (l + a + b)).astype(np.float32), du=(2.0 * rad * a).astype(np.float32), dv=(2.0 * rad * b).astype(np.float32),
                dir=l.astype(np.float32))


def deep_levels(k, tau_max):
    """The k levels (fp32, ascending) of a deep AOV (api.DeepRayAov / DeepViewAov / DeepOrthoAov) that are equally spaced in opacity up to
    optical depth tau_max: alpha_i = (i + 1) / k * (1 - exp(-tau_max)), level i = -log1p(-alpha_i).  Equal steps of alpha are equal steps of
    what a compositor sees; the last level is tau_max itself."""
    k = int(k)
    if not 1 <= k <= 32:
        raise ValueError("deep_levels: 1 .. 32 levels")
    if not (math.isfinite(tau_max) and tau_max > 0.0):
        raise ValueError("deep_levels: tau_max must be finite and positive")
    alpha = (np.arange(1, k + 1, dtype=np.float64) / k) * -np.expm1(-float(tau_max))
    levels = (-np.log1p(-alpha)).astype(np.float32)
    if not (levels[0] > 0.0 and np.isfinite(levels).all() and (np.diff(levels) > 0.0).all()):
        raise ValueError("deep_levels: %d levels up to %g do not separate in fp32" % (k, tau_max))
    return levels


def denoise_params(**kw):
    """The parameters of the denoise filter (api.Denoise / DenoisedFrame / RenderPath(..., denoised_out=); include/nrc_hpm.h, "Denoise") as a
    dict: the defaults -- passes 3, sigma_alpha 0.1, sigma_depth 4.0 (in the units of t), sigma_color +inf (the colour term off),
    color_decay 0.5 -- overridden by the keywords, checked as the library checks them."""
    p = dict(passes=3, sigma_alpha=0.1, sigma_depth=4.0, sigma_color=math.inf, color_decay=0.5)
    for k, v in kw.items():
        if k not in p:
            raise ValueError("denoise_params: unknown parameter %r" % (k,))
        p[k] = int(v) if k == "passes" else float(v)
    if not 1 <= p["passes"] <= 6:
        raise ValueError("denoise_params: passes must be 1 .. 6")
    for k in ("sigma_alpha", "sigma_depth", "sigma_color"):
        if not p[k] > 0.0:      # (NaN included)
            raise ValueError("denoise_params: %s must be > 0 (+inf switches the term off)" % k)
    if not 0.0 < p["color_decay"] <= 1.0:
        raise ValueError("denoise_params: color_decay must lie in (0, 1]")
    return p


def reproject_params(**kw):
    """The parameters of reprojection (api.Reproject / RenderPath(..., accumulated_out=); include/nrc_hpm.h, "Reproject") as a dict: the
    defaults -- max_history 64 (the cap on the frames history may count for), sigma_alpha 0.1, sigma_depth 4.0 (in the units of t) --
    overridden by the keywords, checked as the library checks them."""
    p = dict(max_history=64.0, sigma_alpha=0.1, sigma_depth=4.0)
    for k, v in kw.items():
        if k not in p:
            raise ValueError("reproject_params: unknown parameter %r" % (k,))
        p[k] = float(v)
    if not 0.0 < p["max_history"] < math.inf:      # (NaN included)
        raise ValueError("reproject_params: max_history must be > 0 and finite")
    for k in ("sigma_alpha", "sigma_depth"):
        if not p[k] > 0.0:
            raise ValueError("reproject_params: %s must be > 0 (+inf switches the term off)" % k)
    return p


def deep_tau_bracket(levels, z, flat, depth):
    """What a deep AOV's samples say about the optical depth in front of `depth` -- what a compositor or a shadow look-up does with them.
    levels [K], z [K][...] (the planes), flat [...][4] (the flat result of the same call), depth [...] (an image or array, or a scalar).
    The samples are the knots (z_front, 0), (z[0], L[0]), ..., (z[m - 1], L[m - 1]) of the m finite planes, in depth order, and the total
    tau, which lies somewhere beyond the last knot.  tau(depth) does not decrease, so between knots j - 1 and j it lies in
    [tau_lo, tau_hi] = [tau of knot j - 1, tau of knot j]; in front of z_front it is 0; beyond the last knot it lies in [its tau, total].
    Returns (tau_lo, tau_hi, tau_est) as fp64 arrays of depth's shape: tau_est interpolates linearly in depth between the two knots, and is
    the total beyond the last one (where the samples do not say how far the medium goes on)."""
    L = np.asarray(levels, np.float64).reshape(-1)
    z = np.asarray(z, np.float64)
    flat = np.asarray(flat, np.float64)
    if z.shape[0] != L.size or flat.shape[-1] != 4 or z.shape[1:] != flat.shape[:-1]:
        raise ValueError("deep_tau_bracket: z must be [K][...] and flat [...][4] of the same rays")
    d = np.broadcast_to(np.asarray(depth, np.float64), z.shape[1:])
    total = flat[..., 1]
    knot_t = np.concatenate([flat[..., 2][None], z], axis=0)                               # [K + 1][...], non-decreasing where finite
    knot_tau = np.concatenate([[0.0], L]).reshape((-1,) + (1,) * d.ndim)
    finite = np.isfinite(knot_t)
    m = finite.sum(axis=0)                                                                 # knots a ray has: 0 (saw nothing) .. K + 1
    j = (finite & (knot_t <= d[None])).sum(axis=0)                                         # knots at or in front of depth
    take = lambda a, i: np.take_along_axis(np.broadcast_to(a, knot_t.shape), np.clip(i, 0, L.size)[None], axis=0)[0]
    lo = np.where(j > 0, take(knot_tau, j - 1), 0.0)
    hi = np.where(j == 0, 0.0, np.where(j < m, take(knot_tau, j), total))
    t_lo, t_hi = take(knot_t, j - 1), take(knot_t, j)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(t_hi > t_lo, (d - t_lo) / (t_hi - t_lo), 1.0)
    est = np.where((j > 0) & (j < m), lo + (hi - lo) * np.clip(w, 0.0, 1.0), hi)
    return lo, hi, est


def frame_randoms(n, seed=1337):
    """Per-frame UniformData.random (src/NrcHpmRenderer.cu:308): n x 4 floats in [0,1), seeded (std::mt19937-like role)."""
    rng = np.random.default_rng(seed)
    return rng.random((n, 4), dtype=np.float32)
