'use strict'
// What a document is, through the extension: node test/json.js --cpu|--gpu
//  --cpu : GpuMerge over an engine double built from the bundled yjs; checks what the extension asks of the engine
//          (one jsonMany call per jsonOf; versionJson = restoreVersions, then one jsonMany over the fulfilled results)
//  --gpu : the same through the N-API addon (compat135: the bundle is yjs 13.5.16), string for string against yjs
// A live Tiptap-shaped document (headings with a `level` attr, paragraphs with bold and link marks, edited, with a
// deleted paragraph and an emoji) and a flat Y.Text document: jsonOf equals the restated y-prosemirror serializer
// (tools/json_corpus.js) on the live document; versionJson over three versions equals it on
// Y.createDocFromSnapshot; the Y.Text document asked as a fragment is left out and named.
const path = require('path')
const assert = require('assert')
const { GpuMerge, DocumentStore } = require('../src/index.js')

const mode = process.argv.includes('--gpu') ? 'gpu' : 'cpu'
const TOOLS = path.join(__dirname, '..', '..', '..', 'tools')
const Y = require(path.join(TOOLS, 'yjs_bundle.js')).load()   // the test oracle: yjs from the image's bundle
const { jsonOf, Refuse } = require(path.join(TOOLS, 'json_corpus.js'))   // the committed serializer over yjs's own document

const load = (state, gc) => { const d = new Y.Doc({ gc }); Y.applyUpdate(d, state); return d }
const isNoGc = o => o === 1 || o === true || !!(o && o.gc === false)
const yjsRestore = (state, version, gc) => Y.encodeStateAsUpdate(Y.createDocFromSnapshot(load(state, false), Y.decodeSnapshot(version), new Y.Doc({ gc })))
const restoreOr = (s, v, gc) => { try { return yjsRestore(s, v, gc) } catch (e) { return Object.assign(new Error(String(e.message)), { code: 'EINVAL' }) } }
const jsonOr = (state, name) => { try { return jsonOf(load(state, true), name) } catch (e) { if (!(e instanceof Refuse)) throw e; return Object.assign(new Error('refused'), { code: 'EUNSUPPORTED' }) } }

// test double (never shipped): the engine calls the extension makes, from yjs
class Double {
  constructor () { this.log = [] }
  async mergeUpdates (updates) { return Y.mergeUpdates(updates) }
  async mergeMany (docs) { return docs.map(u => Y.mergeUpdates(u)) }
  async snapshot (update, opts) { return Y.encodeStateAsUpdate(load(update, !(opts && opts.gc === false))) }
  async takeVersionMany (states) { return states.map(s => Y.encodeSnapshot(Y.snapshot(load(s, true)))) }
  async restoreVersionMany (states, versions, opts) { return states.map((s, i) => restoreOr(s, versions[i], !(opts && isNoGc(opts[i])))) }
  async jsonMany (states, names) {
    this.log.push(['jsonMany', states.length, Array.from(names)])
    return states.map((s, i) => jsonOr(s, String(names[i])))
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

function block (frag, at, tag, s, level) {
  const e = new Y.XmlElement(tag)
  frag.insert(at, [e])
  if (tag === 'heading') e.setAttribute('level', level)
  const t = new Y.XmlText()
  e.insert(0, [t])
  t.insert(0, s)
  return t
}

test_('jsonOf and versionJson of a Tiptap-shaped document; a Y.Text document is left out and named', async () => {
  const engine = makeEngine()
  const ext = new GpuMerge({ engine, store: new MemoryStore(), Y })
  try {
    const x = await openDoc(ext, 'tiptap', false, 31)
    const f = await openDoc(ext, 'flat', false, 32)
    const frag = x.document.getXmlFragment('default')
    const now = doc => jsonOf(load(Y.encodeStateAsUpdate(doc), true), 'default')
    const vx = []; const expect = []
    block(frag, 0, 'heading', 'Release notes', 1)
    const p1 = block(frag, 1, 'paragraph', 'The first paragraph 😀 ends here.')
    f.document.getText('default').insert(0, 'flat text')
    vx.push((await ext.takeVersions(['tiptap'])).get('tiptap')); expect.push(now(x.document))
    p1.insert(19, ' (edited)', { bold: true })
    p1.format(4, 5, { link: { href: 'https://example.org/?q="x"', target: null } })
    block(frag, 2, 'paragraph', 'A paragraph that will go.')
    block(frag, 3, 'heading', 'Second "heading"', 2)
    vx.push((await ext.takeVersions(['tiptap'])).get('tiptap')); expect.push(now(x.document))
    frag.delete(2, 1)
    p1.delete(0, 2)
    p1.format(10, 12, { bold: true })
    vx.push((await ext.takeVersions(['tiptap'])).get('tiptap')); expect.push(now(x.document))
    block(frag, 0, 'paragraph', 'Written after the last version.')
    assert.strictEqual(new Set(expect).size, 3)

    // jsonOf: the live documents; the Y.Text document asked as a fragment is refused
    const got = await ext.jsonOf(['tiptap', 'missing', 'flat'])
    assert.deepStrictEqual(Array.from(got.keys()), ['tiptap'])
    assert.strictEqual(got.get('tiptap'), now(x.document))
    assert.deepStrictEqual(ext.unserialized, [{ documentName: 'flat', code: 'EUNSUPPORTED' }])
    const obj = (await ext.jsonOf(['tiptap'], { parse: true })).get('tiptap')
    assert.strictEqual(obj.type, 'doc')
    assert.deepStrictEqual(obj.content[1], { type: 'heading', attrs: { level: 1 }, content: [{ type: 'text', text: 'Release notes' }] })
    const marks = obj.content[2].content.filter(o => o.marks).map(o => o.marks.map(m => m.type).join('+'))
    assert.ok(marks.includes('link') && marks.some(m => m.includes('bold')), JSON.stringify(obj.content[2]))
    assert.deepStrictEqual(obj.content[2].content.find(o => o.marks && o.marks[0].type === 'link').marks[0].attrs, { href: 'https://example.org/?q="x"', target: null })
    assert.strictEqual((await ext.jsonOf(['tiptap'], { field: 'other' })).get('tiptap'), '{"type":"doc","content":[]}')
    if (mode === 'cpu') {
      const calls = engine.log.filter(c => c[0] === 'jsonMany')
      assert.deepStrictEqual(calls, [['jsonMany', 2, ['default', 'default']], ['jsonMany', 1, ['default']], ['jsonMany', 1, ['other']]])
      engine.log.length = 0
    }

    // versionJson: the serializer on Y.createDocFromSnapshot, in entry order; a version ahead of its state rejects alone
    const ahead = Y.encodeSnapshot(Y.createSnapshot(Y.createDeleteSet(), new Map([[31, 100000]])))
    const entries = [{ documentName: 'tiptap', version: vx[2] }, { documentName: 'tiptap', version: ahead }, { documentName: 'tiptap', version: vx[0] },
      { documentName: 'gone', version: vx[0] }, { documentName: 'tiptap', version: vx[1], gc: false }]
    const res = await ext.versionJson(entries)
    assert.deepStrictEqual(res.map(r => r.status), ['fulfilled', 'rejected', 'fulfilled', 'rejected', 'fulfilled'])
    assert.strictEqual(res[1].reason.code, 'EINVAL')
    const at = v => now(Y.createDocFromSnapshot(x.document, Y.decodeSnapshot(v)))
    assert.strictEqual(res[0].value, at(vx[2])); assert.strictEqual(res[0].value, expect[2])
    assert.strictEqual(res[2].value, at(vx[0])); assert.strictEqual(res[2].value, expect[0])
    assert.strictEqual(res[4].value, at(vx[1])); assert.strictEqual(res[4].value, expect[1])
    assert.strictEqual(res[2].value, '{"type":"doc","content":[{"type":"heading","attrs":{"level":1},"content":[{"type":"text","text":"Release notes"}]},' +
      '{"type":"paragraph","content":[{"type":"text","text":"The first paragraph 😀 ends here."}]}]}')
    const parsed = await ext.versionJson(entries.slice(0, 1), { parse: true })
    assert.deepStrictEqual(parsed[0].value, JSON.parse(expect[2]))
    if (mode === 'cpu') assert.deepStrictEqual(engine.log.filter(c => c[0] === 'jsonMany'), [['jsonMany', 3, ['default', 'default', 'default']], ['jsonMany', 1, ['default']]])
  } finally { engine.close() }
})

if (mode === 'gpu') {
  test_('the addon and the pool: strings in caller order, a refused state alone, names as strings or bytes', async () => {
    const { GpuEngine, GpuEnginePool } = require('../src/engine.js')
    const engine = new GpuEngine({ device: 0, compat135: true })
    try {
      const d = new Y.Doc(); d.clientID = 9
      d.getText('tëxt').insert(0, 'héllo wörld')
      block(d.getXmlFragment('default'), 0, 'heading', 'nested', 3)
      const u = Y.encodeStateAsUpdate(d)
      assert.strictEqual(typeof engine.jsonMany, 'function')
      const want = '{"type":"doc","content":[{"type":"heading","attrs":{"level":3},"content":[{"type":"text","text":"nested"}]}]}'
      const r = await engine.jsonMany([u, u.slice(0, u.length - 4), u, u], ['default', 'default', Buffer.from('tëxt'), 'absent'])
      assert.strictEqual(r[0], want)
      assert.ok(r[1] instanceof Error && r[1].code === 'EMALFORMED')
      assert.ok(r[2] instanceof Error && r[2].code === 'EUNSUPPORTED')
      assert.strictEqual(r[3], '{"type":"doc","content":[]}')
      assert.deepStrictEqual(await engine.jsonMany([], []), [])
      await assert.rejects(engine.jsonMany([u], []), x => x.code === 'EINVAL')
      const pool = new GpuEnginePool({ makeEngine: () => engine, devices: [0] })
      assert.deepStrictEqual(await pool.jsonMany(['a', 'b'], [u, u], ['default', 'absent']), [want, '{"type":"doc","content":[]}'])
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
