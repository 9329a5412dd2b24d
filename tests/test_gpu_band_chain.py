"""The band kernels' staging dump slot, hoisted epilogue reads and pinned kernel arguments (apply_band.hip).

The spare LDS slot and the batched epilogue reads can only go wrong where lanes are inactive in the extra-column
staging step or a tile is partial, so every order runs on one element, on a mesh one element row short of a tile
and on one a row past it, and a 3-column strip with both interface lines runs too.  Per shape: the CD operator of
the benchmark, the Laplacian alone and one FULL form (mass, explicit Dirichlet mask with values, accumulate),
with both coefficient modes of the band kernel and with the band-form MFMA kernel.

(a) the preloaded-argument launch, the struct launch, the composition of position-ranged launches and a repeated
    launch are bitwise equal;
(b) max|y - y_ref| <= 1e-13 max|y_ref| against the oracle's CSR operators;
(c) the SHA-256 of y equals the digest of the same seeded case on the commit before the dependent-chain change:
    that change may move waits and loads, never a bit of the result.
DIGESTS was recorded on an MI355X from a build of commit 78f8579: digests(run_case(c)) of every case below.
"""
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-13
PE = 40.0
FORMS = ("cd", "lap", "full")


def band_tye(P):
    """TYE of apply_select.h (band_tye): element rows of a band tile."""
    return max(64 // P, 1)


def shapes(P):
    return [(1, 1), (2, band_tye(P) - 1), (2, band_tye(P) + 1)]


# (P, nex, ney, ex_begin, ex_end): whole meshes of every order
CASES = [(P, nex, ney, 0, nex) for P in range(1, 17) for nex, ney in shapes(P)]
# a middle strip: columns 1..3 of 5, both of its edge lines are interfaces
STRIP_CASES = [(8, 5, 9, 1, 4), (5, 5, 13, 1, 4), (12, 5, 6, 1, 4)]


def case_id(c):
    P, nex, ney, eb, ee = c
    return f"P{P}_{nex}x{ney}" + ("" if (eb, ee) == (0, nex) else f"_strip{eb}-{ee}")


def inputs(c):
    P, nex, ney, eb, ee = c
    n = ((ee - eb) * P + 1) * (ney * P + 1)
    r = np.random.default_rng([P, nex, ney, eb, ee])
    v = {k: r.uniform(-1, 1, n) for k in ("x", "u", "v", "g", "y0")}
    v["mask"] = (r.uniform(0, 1, n) < 0.15).astype(np.uint8)
    return v


def form_kwargs(form, dev):
    from sem_amd import _lib
    if form == "cd":
        return dict(c_stiff=1.0, c_gradx=PE, cu=dev["u"], c_grady=PE, cv=dev["v"], dir_mode=_lib.DIR_IDENTITY,
                    dir_sides=_lib.SIDE_W | _lib.SIDE_E)
    if form == "lap":
        return dict(c_stiff=1.0)
    return dict(c_mass=0.25, c_stiff=1.0, c_gradx=PE, cu=dev["u"], c_grady=PE, cv=dev["v"], c_acc=2.0,
                dir_mode=_lib.DIR_IDENTITY, dir_mask=dev["mask"], dir_val=dev["g"])


def references(c, v):
    """{form: y} from the oracle's assembled CSR operators.  A strip's own elements are a (ncols x ney) mesh of the
    same element size; on its right interface line the pointwise terms and Dirichlet rows belong to the next strip
    (this one leaves 0 in a Dirichlet row there), on its left one to itself."""
    from oracle import sem_oracle as O
    P, nex, ney, eb, ee = c
    nc, dx, dy = ee - eb, 1.0 / nex, 1.5 / ney
    NY = ney * P + 1
    x = v["x"]
    lap = O.global_stiffness_matrix(P, nc, ney, dx, dy) @ x
    Gx, Gy = O.global_gradient_matrices(P, nc, ney, dx, dy)
    conv = lap + PE * v["u"] * (Gx @ x) + PE * v["v"] * (Gy @ x)
    gx = np.arange(x.size) // NY + eb * P
    cd = conv.copy()
    rows = (gx == 0) | (gx == nex * P)
    cd[rows] = x[rows]
    own = ~((gx == ee * P) & (ee < nex))
    full = conv + 0.25 * (O.global_mass_matrix(P, nc, ney, dx, dy) @ x) + np.where(own, 2.0 * v["y0"], 0.0)
    rows = v["mask"] != 0
    full[rows] = np.where(own, x - v["g"], 0.0)[rows]
    return {"cd": cd, "lap": lap, "full": full}


def run_case(c, set_knob):
    """Every launch of one case.  Returns {(form, kernel): [y, ...]} as numpy arrays, kernel in
    'imm' / 'dpp' (band kernel, coefficient mode) / 'mfma'; the list holds the variants that must agree bitwise:
    preloaded-argument launch, repeated launch, struct launch, composed position ranges."""
    from sem_amd import _lib
    from sem_amd.device import get_mesh
    P, nex, ney, eb, ee = c
    mesh = get_mesh(P, nex, ney, 1.0 / nex, 1.5 / ney, eb, ee)
    v = inputs(c)
    dev = {k: mesh.to_device(t, dtype=torch.uint8 if k == "mask" else torch.float64) for k, t in v.items()}
    n = ee - eb
    out = {}
    for form in FORMS:
        kw = form_kwargs(form, dev)

        def launch(**extra):
            return mesh.apply(dev["x"], dev["y0"].clone(), **kw, **extra)

        for name, tile in (("dpp", 3), ("imm", 4)):
            set_knob(_lib.TUNE_BAND_TILE, tile)
            set_knob(_lib.TUNE_BAND_KP, 0)
            ys = [launch(algo=_lib.ALGO_BAND), launch(algo=_lib.ALGO_BAND)]
            set_knob(_lib.TUNE_BAND_KP, -1)
            ys.append(launch(algo=_lib.ALGO_BAND))
            set_knob(_lib.TUNE_BAND_KP, 0)
            y = dev["y0"].clone()
            for pos in [(0, 1), (n, n + 1)] + ([(1, n)] if n > 1 else []):
                mesh.apply(dev["x"], y, pos=pos, algo=_lib.ALGO_BAND, **kw)
            ys.append(y)
            out[form, name] = [t.cpu().numpy() for t in ys]
        out[form, "mfma"] = [launch(algo=_lib.ALGO_MFMA).cpu().numpy() for _ in range(2)]
    return out, v


def sha(ys):
    """SHA-256 over the float64 bytes of the arrays ys, in order."""
    h = hashlib.sha256()
    for y in ys:
        h.update(np.ascontiguousarray(y, dtype=np.float64).tobytes())
    return h.hexdigest()


def digests(out):
    """{kernel: SHA-256 of the y of the three forms (first launch of each), in FORMS order} of run_case's result."""
    return {k: sha([out[form, k][0] for form in FORMS]) for k in ("dpp", "imm", "mfma")}


@pytest.mark.parametrize("c", CASES + STRIP_CASES, ids=case_id)
def test_band_chain(gpu, c, tuning):
    out, v = run_case(c, tuning)
    refs = references(c, v)
    bad = []
    for (form, k), ys in out.items():
        key = f"{case_id(c)}/{form}/{k}"
        for i, y in enumerate(ys[1:], 1):                                   # (a)
            if not np.array_equal(y, ys[0]):
                bad.append(f"{key}: launch variant {i} differs bitwise, max {np.abs(y - ys[0]).max():.3e}")
        err = np.abs(ys[0] - refs[form]).max() / np.abs(refs[form]).max()   # (b)
        print(f"{key}: rel err {err:.3e}")
        if not err <= TOL:
            bad.append(f"{key}: rel err {err:.3e} > {TOL}")
    band, mfma = DIGESTS[case_id(c)]                                        # (c)
    for k, d in digests(out).items():
        want = mfma if k == "mfma" else band
        if d != want:
            bad.append(f"{case_id(c)}/{k}: SHA-256 {d} != recorded {want}")
    assert not bad, "\n".join(bad)


# case: (band kernel, either coefficient mode; band-form MFMA kernel)
DIGESTS = {
    "P1_1x1": ("bd6ff9a9cf606c2d0ea81104f695c918b310b054aeeb863b29924fb84570a09f",
              "ee8a34cfb5b56e6cbe582faadfc376e09b804be9d869dbf91faaee1c86779bfc"),
    "P1_2x63": ("d94046079f1ab80917da26cff7ca88d9e55509193c32d872cfd075efc896cc02",
               "36c3f17d45c737b7a12dffecba5a20792bf4b376f04c4b4ceea43b4cd587347f"),
    "P1_2x65": ("54f0b2d68f56a29b62e237941a1363a1809ca61d06b69948519dbdc019b9b15e",
               "33ebe9041517b79d75cc6cc396f078203ea7a307ce78efae54e371169842bdd6"),
    "P2_1x1": ("8605186531699f31dbff2d418f160fde1fe967002be9e372e36d2a358fc8a083",
              "7150e4473395773093d14a8311822ac75e1175e2c466041e3c69ba24345d7b4c"),
    "P2_2x31": ("88d2f3185b62394990aafcc844e7314a7193897c7b98ceed9f1d4c67e760f3bd",
               "2e1121f8112093e3a338651b6a74a95cf27918922bd06e80040c8ff40c7490cd"),
    "P2_2x33": ("aec7f7f4e86b65b00a8fa0609609b7934fa15986b84d5155db18c602028ac35d",
               "f387edbc441643f64951dae4ce77bc975e51381bf26e176564c9abc5d9bc2c7c"),
    "P3_1x1": ("2c145b4dac177c00a87d5cca4826c9e872223294a2f7dae0b1a67a164b02cbe0",
              "ea2580be3811abb60bb05b1f6570545bf8c51b020bf3c95e86d9237f80bb3509"),
    "P3_2x20": ("1ae70dd0d098d3918a8aa6ce58fec88467564d0c0b15dec0f3d4a4a91f353da9",
               "7469046d33cf0581c67692852d3c3f2de763725971d33dea55f827519e1127b0"),
    "P3_2x22": ("470e3559ee220b1c4e051419a51dc4f5555a735defcdcdf6035ee5627a8f2101",
               "09b3f4fa477f4bafac72069d8455530910026932a5d9c9e4fed287cf6fb21132"),
    "P4_1x1": ("968506dd4d8ecd4a142e7b353781020583697a0a29925444f1ab6165c60aad4c",
              "a060ced2f45257e633961f258bf4313920c143405939c9f41008a548c1408d2b"),
    "P4_2x15": ("adc991b54e8a4de39776a86cc9c85613d9831bea8baa79d9124496978d3fe0c8",
               "1e8b2c9e6e7f7216eb5e42c6e545064ecaac4eae929a36423f1ecfb9bad4d0d1"),
    "P4_2x17": ("531374021d1133ecf53626c354e8bc52574ed66d8e54b9d86e1a4a13702b85e9",
               "8c221ef2b792ee64f9d55d7196318cacb86b13794697e08511f2a293bc63d198"),
    "P5_1x1": ("9b06147f87f78a54f03d3a8a4629b77ef509047fa9b19428bf65c1f9de196418",
              "77e50ce2fee066fdc11a57a8c5ea3dd895f4715859b3b139a329471f1feb74aa"),
    "P5_2x11": ("11a5be214f18214031de3e6ba2a1702712759208f42b821ba60238bcdfa1fcec",
               "fbe8ede3bc247c6d61b52e83ebd80896e4899e43e12e3a21a8b9aecbe4abdbfd"),
    "P5_2x13": ("3787ec7f020b7342d659ca4242e77ba0ffda26bd73686a41b1ef3000af9ddbb9",
               "d634522af8a7afd4731883120d9e9cf535924947ed553b3bcd0f8ec7f9d6a709"),
    "P6_1x1": ("ec71c251fdc3252f2498b656d9e3f85ce72c912f600a15bac606930744a4f53b",
              "2918e9c918a5dbe729f60ac61174361ef9d8b655cb4a68d9ec3c4125fb8038f9"),
    "P6_2x9": ("763ee498de1a162d1ab74cd266f98afb3f2ce2a5202ec07809d2a87600978140",
              "c50899d7b2acdbd28251867e3a3d87fb0eae94bf307bd9ba3f6f9e51c44433aa"),
    "P6_2x11": ("dd6b68a0b6fc89f016854e443af243fc00bf098fe1cdff1d8d829d020e217c4d",
               "332d8f6e048f6eff714232988b2684c944db6096cedeb6d7eaa6f64a3dab9e30"),
    "P7_1x1": ("94c004317a671c9fb74d10830d7d957902eaeffd3cecd2d92dfe6099aa66a60c",
              "0a5cba6d12687bb1638899d52ae4a14b4771994ff88e672bda340e955b870f63"),
    "P7_2x8": ("b9ad48a8e01df2efc5159097bba7e0317be8930c4f9000826f6ccdd6b2ff2c3c",
              "5ffe9184ace25fff145c18aa3eb4fe06e63fe623aa4c0ebb48c8231e391b6bce"),
    "P7_2x10": ("8c2fc041d8b2200296c3f805bc02a5729fc2eb0025486ce5a50d63be779a07d3",
               "aec9117166cff8772b39b1859ddf4984a45945f47573f6d5368ad2fb3363d7af"),
    "P8_1x1": ("987b9ca681a2f4586f17d331a7297f14699d2838ab41c9e2accb90ebcc04fcc5",
              "a295d7ff759ffdbb5ed22781b342ae005c45a6a2b58fb631b00861aaf3011000"),
    "P8_2x7": ("9d93ac1c411a2c9765f2e9905621a471e44882869c1019523ad156c04d3a6601",
              "e7a57f4a1d831c8cc9fa3479ea40a490d0004a48c3061eecc1eea071c0626b71"),
    "P8_2x9": ("d3a5a083b4472868401313df8fc8fc62e6f18c38464e259cda1b753a210f4a3a",
              "7280bee14c8efe4da8ca55be10d214e9a9b2c1fe8e3b57fcfcaf3d1ab5713971"),
    "P9_1x1": ("9ef4fb797ccf51efa7ee4bed863a8d2f8ddf745f50dbeab8c52ccc6e9581fb3a",
              "af8581393fbf612df22be8dc029001edd9e64d3f267027e6ecca6767ec8deedd"),
    "P9_2x6": ("e08f79b04f18496b826575675570d517e0a2bbae357f2f4ed51afd6d3c57478b",
              "dd6ac3d01f7d2ba3bfc7a52f8ae9cc99e4f9bb4d40b2c57eea287931d4b48ec3"),
    "P9_2x8": ("dd26c3bd2c41a9e8ba2fbc517ec32f90f940f0a1998dbcee622aed34c3a72e38",
              "bc9dc6c030e0b771ee4d18066b4a1df8e9f903983a028a313faa9edd02bf1ce1"),
    "P10_1x1": ("dccfdb28305aad717977cfed939dd6fcb8a04f348a209f47ad28a85d7ccfab30",
               "0ce464236370dcd003bb6cef4a269ae74604348621318cda1930ddcdd17803fe"),
    "P10_2x5": ("69f9a4642d80f4fe9b296b89049339f6405d4d5dabbae7fa2be85d773c70576f",
               "d05af3afd997a1e26513f8d6f6c2aa76fb42189f8e9b6909cdec770681b94b88"),
    "P10_2x7": ("a6bd75fd5e1e25c2f50973c6a55c1141217f2f05af9d7950728ce396d8928413",
               "d1483d0699090a903e9751e864b47118f6ca37f160df717aa3d7f45d4633aa68"),
    "P11_1x1": ("8784aa168bce7f7870beda604264e6f4320b91373da2e540481f6a2e1d80f29a",
               "26b092d8188d31da1fb91c2b2ea369add903445137631be8c4e6901b51a95b14"),
    "P11_2x4": ("29319ffeb165ebb9ef5ae63949dd00822942ab8e66afe3d47e716c61552de017",
               "0697ce5d0db20251f655a00957aa2ea623844b836bb3d0a7adfe57e0feaf1871"),
    "P11_2x6": ("f9e041306f9f8758e91f74bba83398d34e53d391b9b81048ab231eb0ee6f978d",
               "210f825b3acd7f26fe41e9d9851e45255380af847a61bc218ac57143bb536c8d"),
    "P12_1x1": ("f44d1f66adf503a95e0b4fc1c861331f9d34811474b37076ef0a5d0b9a797e70",
               "7f407501fd1c0b76f43f96c50da470f590f0fdadb9dbb1db728553c1cfa7b72a"),
    "P12_2x4": ("dedc9d5cf79c14b5ffd2bc2d002b0f8f553eb5231d9c6212af6ab5cd80def840",
               "d5fd60810b46d2cf4c47ac9cd1b9704fb819fc09161fbd195dbcf15dc57a053d"),
    "P12_2x6": ("ee1afe432066f7b5a0c90b6ff6ae91d81ecee63fde4cebc3503394550a935dff",
               "0bc808c6b2293e41dbcb6de753542c9824842a16e4fd6faf804724b6eae3af6d"),
    "P13_1x1": ("2fb4acbea85fe7ff45f78ced4e61d87e4f4667cbf74ad082262cc075c0b52341",
               "6442b5db116be9b9c4362a823549e9ec5cccddaeccd7be9fb9bf2dfa85168eee"),
    "P13_2x3": ("fc94419cb5f8faae179b6e042692b75e8b5521dbb89fdd0297bc4fbdd8327fcd",
               "d3d71091115ee89562a92b8c63d38823644b318950077d6987c0928ade4b5139"),
    "P13_2x5": ("9196e6d8aaeb8a8af12bc8598a3dd49bc6a9852f40d36a36e6431d2f62c6d6b5",
               "4dc6457e0cf579a9b0b0abe644298aaf9cd119e83c2c7976262f355607e51795"),
    "P14_1x1": ("5e5e31ba3df498d9dd2a66d6b0c90bac6604af299a0523c5b8c557bace661a0a",
               "f843ef8c7ef2d32935abf5bf94d73ec93263785d1116fce5e502bf385bfe2d9f"),
    "P14_2x3": ("a19291a5ddf0d8e015ebbd060911128752a4c4caba3ec6c8c29a2908a086a66e",
               "0adcf88be7bd0bdcf2281717f8526e5c9424fd99388ad6498030de7f461f64c1"),
    "P14_2x5": ("4cf1f3b8bd9ddb6de81d509bd01dab2a47fcd4c23e9d7ef11fb3c1166252b70a",
               "edf98749bfe066732378f2fdfce892b4724b9b003ecedf7806ad932beed73054"),
    "P15_1x1": ("923948fecc434dcdebfc64c302ae15df54daa7cbb66b16502ca15093b9da774a",
               "dcb6b36323bbf3b1b0a2409e6825ba28fb4affe72f28ed423391c4cb29b84004"),
    "P15_2x3": ("32b7db69c62e1128fcaf3d2f43693f44e36fc401561bae615cfa4a0b75802176",
               "04e545bbe5743ac59e9002ad97bb79128a425b57199eb4b53b898034d46b0db7"),
    "P15_2x5": ("132ca248c5b10a34e7b930e6276c329c7d00f5093ef84fc6fa77f087ca9c5c79",
               "71397487c1fe16ff9740990729bfa3a0c30a24fb67dd2b8e7a2a72d291283b43"),
    "P16_1x1": ("a960c129b779a1d7861460a4e03d58387410eff65aa077ca91bdf21e0e8b2f20",
               "3c8c1cd7ee36a3ca2df82f1a9b2de2a8308408c88b7d9131e185844ef4cddc77"),
    "P16_2x3": ("c083e957075ed643bde4ac22825a757eb9e60f26028f646ece775ab7bc8a5944",
               "56e707979e848297c549fece696cef9164939da84d68bab41e6ec2b0640a55e2"),
    "P16_2x5": ("4b764cedda3e0fc5829782a666c9f33434c71e70a3040339aa308a430627760f",
               "1ebd04ecbdf77bf06f015ef33f817558d49a3831b4b0fd6943f79755d5449672"),
    "P8_5x9_strip1-4": ("fcee71519960bfd35ce4f013ae2384b300efa3cd207b069081633f7a20887a0e",
                       "2d6c62887970e31d18cd07048117856855a0741dd8f00251dbdec8121fd52cb4"),
    "P5_5x13_strip1-4": ("92f62e138588c6693a57799a07a0d07ffd6ea0ae05a11c31ddf752ed4fa99627",
                        "efc90547827289762d488776731d820534e61be1eb1ca8bf0f5037e3e4efffb9"),
    "P12_5x6_strip1-4": ("854bb4a1aa0be48e19e69ef3583e12b4f5d74fe203b01290876074e065762ef3",
                        "9d3db5b5287de5415dbee6124e861aa0840dac43ad8cc1c82c89d86ccbe68892"),
}
