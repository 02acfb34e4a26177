"""The drop-in recipe of INTEGRATION.md §2 (CPU).  The caller's tree is a stand-in written by the `caller_src` fixture in the
reference's src/ layout: `model/`, `components/`, `utils/` as namespace packages, the scripts' import blocks in their files.  The
modules this package must SHADOW (model.DiTTO, model.SpeechGenerator, model.SpeechLP, components.DiT, components.VectorQuantizer)
raise on import, so a recipe that lets one of them win fails loudly; the ones that must FALL THROUGH to the caller's tree
(utils.*, model.NeuralAudioCodec, components.EnCodec) are small modules whose __file__ is checked.  Each case runs in a fresh
interpreter so sys.path / sys.modules start clean."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHADOWED = ("model/DiTTO.py", "model/SpeechLP.py", "components/DiT.py", "components/VectorQuantizer.py")
CALLER_FILES = {
    "utils/Config.py": '''
        class BaseConfig:
            SAMPLE_RATE = 24000


        class ConfigDiTTO(BaseConfig):
            MODEL_NAME = "DiTTO"
            HIDDEN_DIM = 256
            NUM_LAYERS = 2
            NUM_HEADS = 4
            TIME_DIM = 256
            TEXT_EMBED_DIM = 256
            DIFFUSION_STEPS = 50

            @classmethod
            def display(cls):
                print("DiTTO Settings:", {k: v for k, v in vars(cls).items() if k.isupper()})


        class ConfigNAC(BaseConfig):
            LAMBDA_FACTOR = 0.1

            @classmethod
            def display(cls):
                print("NAC Settings:", cls.LAMBDA_FACTOR)


        class ConfigSLP(BaseConfig):
            NB_CLASSES = 11
            NUM_HEADS = 1
            NUM_LAYERS = 1
            EMBEDDING_DIM = 64

            @classmethod
            def display(cls):
                print("SLP Settings:", cls.NB_CLASSES)
    ''',
    "utils/Trainer.py": '''
        class Trainer:
            def set_model(self, model, name):
                self.model, self.name = model, name
                return self
    ''',
    "utils/MLS.py": "MLS = object\n",
    "model/NeuralAudioCodec.py": "class NAC:\n    pass\n",
    "components/EnCodec.py": "class EnCodec:\n    pass\n",
    # the scripts' import blocks come first, ended by a marker line; what follows must never run
    "TrainDiTTO.py": '''
        from model.DiTTO import DiTTO
        from utils.Config import ConfigDiTTO, ConfigNAC
        from utils.Trainer import Trainer
        from utils.MLS import MLS
        ConfigDiTTO.display()
        # --- end of import block
        raise SystemExit("the stand-in script body is not part of the test")
    ''',
    "model/SpeechGenerator.py": '''
        import torch
        from model.DiTTO import DiTTO
        from model.SpeechLP import SLP
        from utils.Config import ConfigDiTTO, ConfigSLP
        # --- end of import block
        raise ImportError("the caller's model.SpeechGenerator was imported: this package's alias should have won")
    ''',
}


@pytest.fixture
def caller_src(tmp_path):
    src = tmp_path / "src"
    for rel, body in CALLER_FILES.items():
        (src / rel).parent.mkdir(parents=True, exist_ok=True)
        (src / rel).write_text(textwrap.dedent(body).lstrip())
    for rel in SHADOWED:
        mod = rel[:-3].replace("/", ".")
        (src / rel).write_text(f"raise ImportError('the caller\\'s {mod} was imported: this package\\'s alias should have won')\n")
    return str(src)


def import_block(path):
    lines = open(path).read().splitlines()
    return "\n".join(lines[:lines.index("# --- end of import block")])


def run(body, cwd=None):
    code = textwrap.dedent(body)
    env = dict(os.environ, PYTHONPATH="")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=cwd or ROOT, env=env,
                       timeout=600)
    assert r.returncode == 0, f"stdout:\n{r.stdout[-3000:]}\nstderr:\n{r.stderr[-3000:]}"
    return r.stdout


def test_traindito_import_block_under_the_recipe(caller_src):
    """sys.path exactly as INTEGRATION.md §2, then the caller script's import block, then the constructor call with the
    codec escape."""
    src = import_block(os.path.join(caller_src, "TrainDiTTO.py"))
    assert "from utils.Trainer import Trainer" in src and "ConfigDiTTO.display()" in src
    out = run(f"""
        import sys
        sys.path.insert(0, {caller_src!r})                         # the caller's tree (scripts run from src/)
        sys.path.insert(0, {ROOT!r})                               # the package
        sys.path.insert(0, {os.path.join(ROOT, "ditto_tts_amd", "compat")!r})
        exec(compile({src!r}, "TrainDiTTO.py:import block", "exec"))
        import ditto_tts_amd.modules as M, utils.Config, utils.Trainer, utils.MLS
        assert DiTTO is M.DiTTO, DiTTO
        assert utils.Config.__file__.startswith({caller_src!r}), utils.Config.__file__
        assert utils.Trainer.__file__.startswith({caller_src!r}) and utils.MLS.__file__.startswith({caller_src!r})
        assert ConfigNAC.LAMBDA_FACTOR == 0.1
        # modules.py's own `from model.NeuralAudioCodec import NAC` resolves to the caller's tree too
        import model.NeuralAudioCodec as NACmod
        assert NACmod.__file__.startswith({caller_src!r})
        from components.DiT import DiT, GlobalAdaLN, RotaryEmbedding
        assert DiT is M.DiT and GlobalAdaLN is M.GlobalAdaLN
        from components.VectorQuantizer import VectorQuantizer
        import ditto_tts_amd.around as A
        assert VectorQuantizer is A.VectorQuantizer
        import components.EnCodec as E
        assert E.__file__.startswith({caller_src!r})
        m = DiTTO(hidden_dim=ConfigDiTTO.HIDDEN_DIM, num_layers=1, num_heads=ConfigDiTTO.NUM_HEADS,
                  time_dim=ConfigDiTTO.TIME_DIM, text_dim=ConfigDiTTO.TEXT_EMBED_DIM, diffusion_steps=20,
                  nac_model_path=None)
        t = Trainer().set_model(m, name=ConfigDiTTO.MODEL_NAME)
        print("ok-train")
    """)
    assert "DiTTO Settings" in out and "ok-train" in out


def test_speechgenerator_import_block_and_config_mutation(caller_src):
    """The caller's model/SpeechGenerator.py import block under the recipe; then a notebook's flow: mutate ConfigDiTTO on the
    caller's module, build the sampler, and the loop length follows the caller's global at call time."""
    src = import_block(os.path.join(caller_src, "model", "SpeechGenerator.py"))
    assert "from model.SpeechLP import SLP" in src and "from utils.Config import ConfigDiTTO, ConfigSLP" in src
    out = run(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import ditto_tts_amd.compat as compat
        compat.install(reference_src={caller_src!r})
        exec(compile({src!r}, "SpeechGenerator.py:import block", "exec"))
        import ditto_tts_amd.modules as M, ditto_tts_amd.slp as S, ditto_tts_amd.sampler as P
        assert DiTTO is M.DiTTO and SLP is S.SLP
        from model.SpeechGenerator import SpeechGenerator
        assert SpeechGenerator is P.SpeechGenerator
        from utils.Config import ConfigSLP, ConfigNAC, ConfigDiTTO
        assert sys.modules["utils.Config"].__file__.startswith({caller_src!r})
        ConfigSLP.display(); ConfigNAC.display(); ConfigDiTTO.display()
        ConfigDiTTO.DIFFUSION_STEPS = 40
        ConfigDiTTO.NUM_LAYERS = 1
        sg = SpeechGenerator(lambda_factor=ConfigNAC.LAMBDA_FACTOR, nac_model_path=None, ditto_model_path=None,
                             slp_path=None, sample_rate=ConfigNAC.SAMPLE_RATE, device="cpu")
        assert sg.ditto_model.cfg.diffusion_steps == 40 and len(sg.betas) == 40 and sg._loop_steps() == 40
        assert sg.ditto_model.cfg.hidden_dim == ConfigDiTTO.HIDDEN_DIM and sg.ditto_model.cfg.num_layers == 1
        ConfigDiTTO.DIFFUSION_STEPS = 25                  # mutated after construction: read at call time
        assert sg._loop_steps() == 25
        ConfigDiTTO.DIFFUSION_STEPS = 1000
        try:
            sg._loop_steps(); raise SystemExit("expected IndexError")
        except IndexError:
            pass
        pinned = SpeechGenerator(ditto_model=sg.ditto_model, device="cpu", diffusion_steps=10)
        assert pinned._loop_steps() == 10
        print("ok-sampler")
    """)
    assert "ok-sampler" in out


def test_unmodified_script_through_the_launcher(caller_src, tmp_path):
    """`python -m ditto_tts_amd.run_reference <script>`: a script that sits in the caller's src/ layout and uses its import
    lines runs unchanged (sys.path[0] = its directory would otherwise make src/model/DiTTO.py win)."""
    script = os.path.join(caller_src, "script.py")
    with open(script, "w") as f:
        f.write(textwrap.dedent("""
            from model.DiTTO import DiTTO
            from utils.Config import ConfigDiTTO, ConfigNAC
            from utils.Trainer import Trainer
            import model.DiTTO as md, sys
            print("DITTO_FROM", md.__file__)
            print("ARGS", sys.argv[1:])
        """))
    code = f"import sys; sys.path.insert(0, {ROOT!r}); sys.argv = ['x', {script!r}, '--flag']\n" \
           "from ditto_tts_amd.run_reference import main; main(sys.argv[1:])\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.join("ditto_tts_amd", "compat", "model", "DiTTO.py") in r.stdout and "ARGS ['--flag']" in r.stdout
