"""The ops package keeps one surface: what a submodule defines is what ``ops.<name>`` gives, and nothing is defined twice.
No GPU and no library load: the modules are only imported."""
import importlib
import pkgutil
import types


def _defined_public(mod):
    """Public names a module defines itself: its functions and classes, and its upper-case constants."""
    out = {}
    for name, v in vars(mod).items():
        if name.startswith("_") or isinstance(v, types.ModuleType):
            continue
        if (getattr(v, "__module__", None) == mod.__name__) if callable(v) else name.isupper():
            out[name] = v
    return out


def test_every_public_name_of_a_submodule_is_the_package_attribute(dfepe):
    ops = dfepe.ops
    owner = {}
    for info in pkgutil.iter_modules(ops.__path__):
        mod = importlib.import_module(ops.__name__ + "." + info.name)
        names = _defined_public(mod)
        if not info.name.startswith("_"):
            assert names, f"ops.{info.name} defines nothing public"
        for name, v in names.items():
            assert name not in owner, f"{name} is defined in ops.{owner.get(name)} and in ops.{info.name}"
            owner[name] = info.name
            assert getattr(ops, name, None) is v, f"ops.{name} is not what ops.{info.name} defines"
    assert len(owner) >= 75  # the surface when the file became a package
    for name in ("_ptr", "_stream", "_on", "_prep", "_t_arg", "_floss_args"):  # private names the package's other files and tests use
        assert callable(getattr(ops, name))
    assert ops._lib is dfepe._lib
