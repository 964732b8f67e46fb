'use strict'
// What a document says, through the extension: node test/text.js --cpu|--gpu
//  --cpu : GpuMerge over an engine double built from the bundled yjs; checks what the extension asks of the engine
//          (one textMany call per textOf; versionTexts = restoreVersions, then one textMany over the fulfilled results)
//  --gpu : the same through the N-API addon (compat135: the bundle is yjs 13.5.16), string for string against yjs
// A live Tiptap-shaped document (paragraphs and headings of XmlText under the XmlFragment 'default', edited, with a
// deleted paragraph and an emoji) and a flat Y.Text document: textOf equals the walker / toString() on the live
// documents; versionTexts over three versions equals the walker on Y.createDocFromSnapshot; a version ahead of its
// state rejects alone.
const path = require('path')
const assert = require('assert')
const { GpuMerge, DocumentStore } = require('../src/index.js')

const mode = process.argv.includes('--gpu') ? 'gpu' : 'cpu'
const TOOLS = path.join(__dirname, '..', '..', '..', 'tools')
const Y = require(path.join(TOOLS, 'yjs_bundle.js')).load()   // the test oracle: yjs from the image's bundle
const { deepText } = require(path.join(TOOLS, 'text_corpus.js'))   // the committed walker over yjs's integrated document

const load = (state, gc) => { const d = new Y.Doc({ gc }); Y.applyUpdate(d, state); return d }
const isNoGc = o => o === 1 || o === true || !!(o && o.gc === false)
const yjsRestore = (state, version, gc) => Y.encodeStateAsUpdate(Y.createDocFromSnapshot(load(state, false), Y.decodeSnapshot(version), new Y.Doc({ gc })))
const restoreOr = (s, v, gc) => { try { return yjsRestore(s, v, gc) } catch (e) { return Object.assign(new Error(String(e.message)), { code: 'EINVAL' }) } }

// test double (never shipped): the engine calls the extension makes, from yjs
class Double {
  constructor () { this.log = [] }
  async mergeUpdates (updates) { return Y.mergeUpdates(updates) }
  async mergeMany (docs) { return docs.map(u => Y.mergeUpdates(u)) }
  async snapshot (update, opts) { return Y.encodeStateAsUpdate(load(update, !(opts && opts.gc === false))) }
  async takeVersionMany (states) { return states.map(s => Y.encodeSnapshot(Y.snapshot(load(s, true)))) }
  async restoreVersionMany (states, versions, opts) { return states.map((s, i) => restoreOr(s, versions[i], !(opts && isNoGc(opts[i])))) }
  async textMany (states, names, { deep = false } = {}) {
    this.log.push(['textMany', states.length, Array.from(names), deep])
    return states.map((s, i) => { const t = load(s, true).getText(String(names[i])); return deep ? deepText(t) : t.toString() })
  }
  close () {}
}

class MemoryStore extends DocumentStore {
  constructor () { super(); this.rows = new Map() }
  async fetchMany (payloads) { return payloads.map(p => this.rows.get(p.documentName) || null) }
  async storeMany (entries) { for (const e of entries) this.rows.set(e.payload.documentName, Uint8Array.from(e.state)) }
}

async function openDoc (ext, name, gc, id) {
  const document = new Y.Doc({ gc })
  document.clientID = id
  document.name = name
  const payload = { document, documentName: name, context: {}, requestParameters: new Map() }
  await ext.onLoadDocument(payload)
  await ext.afterLoadDocument(payload)
  return payload
}

function makeEngine () {
  if (mode === 'cpu') return new Double()
  const { GpuEngine } = require('../src/engine.js')
  return new GpuEngine({ device: 0, batchWindowMs: 5, compat135: true })
}

function block (frag, at, tag, s) {
  const e = new Y.XmlElement(tag)
  frag.insert(at, [e])
  if (tag === 'heading') e.setAttribute('level', '2')
  const t = new Y.XmlText()
  e.insert(0, [t])
  t.insert(0, s)
  return t
}

test_('textOf and versionTexts of a Tiptap-shaped and a flat document', async () => {
  const engine = makeEngine()
  const ext = new GpuMerge({ engine, store: new MemoryStore(), Y })
  try {
    const x = await openDoc(ext, 'tiptap', false, 31)
    const f = await openDoc(ext, 'flat', false, 32)
    const frag = x.document.getXmlFragment('default')
    const ft = f.document.getText('t')
    const walk = doc => deepText(doc.getXmlFragment('default'))
    const vx = []; const expect = []
    // three versions between edits
    block(frag, 0, 'heading', 'Release notes')
    const p1 = block(frag, 1, 'paragraph', 'The first paragraph 😀 ends here.')
    ft.insert(0, 'flat text, first line\n')
    vx.push((await ext.takeVersions(['tiptap'])).get('tiptap')); expect.push(walk(x.document))
    p1.insert(19, ' (edited)', { bold: true })
    block(frag, 2, 'paragraph', 'A paragraph that will go.')
    block(frag, 3, 'paragraph', '')
    block(frag, 4, 'paragraph', 'The last one.\n')
    vx.push((await ext.takeVersions(['tiptap'])).get('tiptap')); expect.push(walk(x.document))
    frag.delete(2, 1)
    p1.delete(4, 6)
    ft.insert(ft.length, 'second 🎉 line'); ft.delete(0, 5)
    vx.push((await ext.takeVersions(['tiptap'])).get('tiptap')); expect.push(walk(x.document))
    block(frag, 0, 'paragraph', 'Written after the last version.')
    assert.strictEqual(new Set(expect).size, 3)

    // textOf: the live documents, deep (the default) and flat
    const deepNow = await ext.textOf(['tiptap', 'missing', 'flat'])
    assert.deepStrictEqual(Array.from(deepNow.keys()), ['tiptap', 'flat'])
    assert.strictEqual(deepNow.get('tiptap'), walk(x.document))
    assert.ok(deepNow.get('tiptap').startsWith('Written after the last version.\nRelease notes\nThe paragraph (edited) 😀 ends here.\n'))
    assert.strictEqual(deepNow.get('flat'), '')   // the flat document has no root 'default'
    const flatNow = await ext.textOf(['flat', 'tiptap'], { field: 't', deep: false })
    assert.strictEqual(flatNow.get('flat'), f.document.getText('t').toString())
    assert.strictEqual(flatNow.get('flat'), 'text, first line\nsecond 🎉 line')
    assert.strictEqual(flatNow.get('tiptap'), '')
    assert.strictEqual((await ext.textOf(['tiptap'], { deep: false })).get('tiptap'), load(Y.encodeStateAsUpdate(x.document), true).getText('default').toString())
    assert.strictEqual((await ext.textOf(['flat'], { field: 't' })).get('flat'), deepText(f.document.getText('t')))
    if (mode === 'cpu') {
      const calls = engine.log.filter(c => c[0] === 'textMany')
      assert.deepStrictEqual(calls[0], ['textMany', 2, ['default', 'default'], true])
      assert.deepStrictEqual(calls[1], ['textMany', 2, ['t', 't'], false])
      engine.log.length = 0
    }

    // versionTexts: the walker on Y.createDocFromSnapshot, in entry order; a version ahead of its state rejects alone
    const ahead = Y.encodeSnapshot(Y.createSnapshot(Y.createDeleteSet(), new Map([[31, 100000]])))
    const entries = [{ documentName: 'tiptap', version: vx[2] }, { documentName: 'tiptap', version: ahead }, { documentName: 'tiptap', version: vx[0] },
      { documentName: 'gone', version: vx[0] }, { documentName: 'tiptap', version: vx[1], gc: false }]
    const res = await ext.versionTexts(entries)
    assert.deepStrictEqual(res.map(r => r.status), ['fulfilled', 'rejected', 'fulfilled', 'rejected', 'fulfilled'])
    assert.strictEqual(res[1].reason.code, 'EINVAL')
    const at = v => walk(Y.createDocFromSnapshot(x.document, Y.decodeSnapshot(v)))
    assert.strictEqual(res[0].value, at(vx[2])); assert.strictEqual(res[0].value, expect[2])
    assert.strictEqual(res[2].value, at(vx[0])); assert.strictEqual(res[2].value, expect[0])
    assert.strictEqual(res[4].value, at(vx[1])); assert.strictEqual(res[4].value, expect[1])
    assert.strictEqual(res[2].value, 'Release notes\nThe first paragraph 😀 ends here.\n')
    if (mode === 'cpu') assert.deepStrictEqual(engine.log.filter(c => c[0] === 'textMany'), [['textMany', 3, ['default', 'default', 'default'], true]])
  } finally { engine.close() }
})

if (mode === 'gpu') {
  test_('the addon and the pool: strings in caller order, a refused state alone, names as strings or bytes', async () => {
    const { GpuEngine, GpuEnginePool } = require('../src/engine.js')
    const engine = new GpuEngine({ device: 0, compat135: true })
    try {
      const d = new Y.Doc(); d.clientID = 9
      d.getText('tëxt').insert(0, 'héllo wörld')
      block(d.getXmlFragment('default'), 0, 'paragraph', 'nested')
      const u = Y.encodeStateAsUpdate(d)
      assert.strictEqual(typeof engine.textMany, 'function')
      const r = await engine.textMany([u, u.slice(0, u.length - 4), u, u], ['tëxt', 'tëxt', Buffer.from('default'), 'absent'])
      assert.strictEqual(r[0], 'héllo wörld')
      assert.ok(r[1] instanceof Error && r[1].code === 'EMALFORMED')
      assert.strictEqual(r[2], ''); assert.strictEqual(r[3], '')
      const deep = await engine.textMany([u, u], ['default', 'tëxt'], { deep: true })
      assert.deepStrictEqual(deep, ['nested\n', 'héllo wörld'])
      assert.deepStrictEqual(await engine.textMany([], []), [])
      await assert.rejects(engine.textMany([u], []), x => x.code === 'EINVAL')
      const pool = new GpuEnginePool({ makeEngine: () => engine, devices: [0] })
      assert.deepStrictEqual(await pool.textMany(['a', 'b'], [u, u], ['default', 'tëxt'], { deep: true }), deep)
    } finally { engine.close() }
  })
}

function test_ (name, fn) { (test_.all = test_.all || []).push({ name, fn }) }

;(async () => {
  let failed = 0
  for (const t of test_.all) {
    try { await t.fn(); console.log('ok   ' + t.name) } catch (e) { failed++; console.log('FAIL ' + t.name + '\n' + (e && e.stack || e)) }
  }
  console.log(failed ? failed + ' failed' : test_.all.length + ' passed (' + mode + ')')
  process.exit(failed ? 1 : 0)
})()
